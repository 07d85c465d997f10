"""The wire form of an issue resolution (gyeeta_amd/wire.py: MM_LISTENER_ISSUE_RESOL, DOWNSTREAM_ONE, resol_messages) without a GPU: the two
numpy layouts against the same structs restated in a small C program compiled here (sizes and every member offset as the compiler lays
them out), and resol_messages on a hand-made set of host-form rows."""
import os
import subprocess

import numpy as np

from gyeeta_amd import wire
from gyeeta_amd.engine import SketchEngine

C_SRC = r"""
#include <stdbool.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
struct down_one {
	uint8_t downstream_glob_id_buf[8];
	uint8_t downstream_state, downstream_issue, downstream_issue_bit_hist, src_upstream_tier;
};
struct resol {
	_Alignas(8) uint64_t issue_src_glob_id;
	uint64_t issue_src_madhava_id, issue_src_time_usec;
	char issue_src_comm[16];
	uint16_t ndownstreams;
	bool src_is_load_balanced;
	uint8_t src_state, src_issue, issue_bit_hist, padding_len;
};
#define F(s, m) printf(#s "." #m " %zu\n", offsetof(struct s, m))
int main(void)
{
	printf("resol %zu %zu\ndown_one %zu %zu\n", sizeof(struct resol), _Alignof(struct resol), sizeof(struct down_one), _Alignof(struct down_one));
	F(resol, issue_src_glob_id); F(resol, issue_src_madhava_id); F(resol, issue_src_time_usec); F(resol, issue_src_comm); F(resol, ndownstreams);
	F(resol, src_is_load_balanced); F(resol, src_state); F(resol, src_issue); F(resol, issue_bit_hist); F(resol, padding_len);
	F(down_one, downstream_glob_id_buf); F(down_one, downstream_state); F(down_one, downstream_issue); F(down_one, downstream_issue_bit_hist);
	F(down_one, src_upstream_tier);
	return 0;
}
"""


def test_layouts_match_the_compiler(tmp_path):
    src, exe = tmp_path / "resol.c", tmp_path / "resol"
    src.write_text(C_SRC)
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", str(src), "-o", str(exe)])
    lines = [ln.split() for ln in subprocess.check_output([str(exe)]).decode().splitlines()]
    assert lines[0] == ["resol", str(wire.MM_LISTENER_ISSUE_RESOL.itemsize), "8"] and lines[1] == ["down_one", str(wire.DOWNSTREAM_ONE.itemsize), "1"]
    dts = {"resol": wire.MM_LISTENER_ISSUE_RESOL, "down_one": wire.DOWNSTREAM_ONE}
    seen = set()
    for name, off in lines[2:]:
        st, f = name.split(".")
        assert dts[st].fields[f][1] == int(off), name
        seen.add(name)
    assert {"resol." + n for n in wire.MM_LISTENER_ISSUE_RESOL.names if n != "tail_pad"} | {"down_one." + n for n in wire.DOWNSTREAM_ONE.names} == seen
    assert wire.MAX_DOWNSTREAM_TIERS == 8 and wire.MAX_DOWNSTREAM_IDS == 2048


def _row(slot, role, src=0xFFFFFFFF, via=0xFFFFFFFF, tier=0, state=3, issue=7, nresolved=0):
    r = np.zeros(1, dtype=SketchEngine.SVC_RESOL_ROW_DT)[0]
    r["glob_id"], r["slot"], r["role"], r["src_slot"], r["via_slot"], r["tier"], r["state"], r["issue"], r["nresolved"] = 0xAB00000000 + slot, slot, role, src, via, tier, state, issue, nresolved
    if src != 0xFFFFFFFF:
        r["src_glob_id"] = 0xAB00000000 + src
    return r


def _parse(payload, nmsg):
    out, at = [], 0
    for _ in range(nmsg):
        hdr = np.frombuffer(payload, dtype=wire.MM_LISTENER_ISSUE_RESOL, count=1, offset=at)[0]
        n = int(hdr["ndownstreams"])
        one = np.frombuffer(payload, dtype=wire.DOWNSTREAM_ONE, count=n, offset=at + 48)
        assert at % 8 == 0 and int(hdr["padding_len"]) == -(48 + 12 * n) % 8
        pad = payload[at + 48 + 12 * n:at + 48 + 12 * n + int(hdr["padding_len"])]
        assert pad == b"\0" * len(pad)
        out.append((hdr, one))
        at += 48 + 12 * n + int(hdr["padding_len"])
    assert at == len(payload)
    return out


def test_resol_messages_on_a_hand_made_row_set():
    # sources 9 (three reached: a carrier at tier 1, resolved at tiers 1 and 2), 4 (one resolved), 20 (nothing reached); an unresolved slot
    rows = np.array([_row(30, 2, src=9, via=12, tier=2), _row(9, 1, src=9, state=4, issue=2, nresolved=2), _row(12, 3, src=9, via=9, tier=1, state=2, issue=0),
                     _row(11, 2, src=9, via=9, tier=1, state=5), _row(4, 1, src=4, state=3, issue=1, nresolved=1), _row(5, 2, src=4, via=4, tier=1),
                     _row(20, 1, src=20, state=3, issue=3), _row(40, 4)], dtype=SketchEngine.SVC_RESOL_ROW_DT)
    payload, nmsg = wire.resol_messages(rows, madhava_id=0x77, time_usec=123456, comm=b"nginx")
    assert nmsg == 2 and len(payload) == (48 + 12 + 4) + (48 + 36 + 4)
    (h4, d4), (h9, d9) = _parse(payload, nmsg)
    assert (int(h4["issue_src_glob_id"]), int(h4["ndownstreams"]), int(h4["src_state"]), int(h4["src_issue"]), int(h4["padding_len"])) == (0xAB00000004, 1, 3, 1, 4)
    assert (int(h9["issue_src_glob_id"]), int(h9["ndownstreams"]), int(h9["src_state"]), int(h9["src_issue"]), int(h9["padding_len"])) == (0xAB00000009, 3, 4, 2, 4)
    assert int(h9["issue_src_madhava_id"]) == 0x77 and int(h9["issue_src_time_usec"]) == 123456 and h9["issue_src_comm"] == b"nginx" and not h9["src_is_load_balanced"]
    ids = lambda d: [int(x) for x in d["downstream_glob_id_buf"].copy().view("<u8").ravel()]
    assert ids(d4) == [0xAB00000005] and [int(t) for t in d4["src_upstream_tier"]] == [1]
    assert ids(d9) == [0xAB0000000B, 0xAB0000000C, 0xAB0000001E] and [int(t) for t in d9["src_upstream_tier"]] == [1, 1, 2]
    assert [int(s) for s in d9["downstream_state"]] == [5, 2, 3] and [int(s) for s in d9["downstream_issue"]] == [7, 0, 7] and not d9["downstream_issue_bit_hist"].any()
    # two dependents: 48 + 24 = 72 bytes, no padding
    payload, nmsg = wire.resol_messages(rows[[1, 2, 3]])
    assert nmsg == 1 and len(payload) == 72 and int(_parse(payload, 1)[0][0]["padding_len"]) == 0
    # more dependents than one element holds: the source is named again
    many = np.array([_row(1, 1, src=1, state=3, issue=1)] + [_row(100 + i, 2, src=1, via=1, tier=1) for i in range(wire.MAX_DOWNSTREAM_IDS + 5)], dtype=SketchEngine.SVC_RESOL_ROW_DT)
    payload, nmsg = wire.resol_messages(many)
    parts = _parse(payload, nmsg)
    assert nmsg == 2 and [int(h["ndownstreams"]) for h, _ in parts] == [wire.MAX_DOWNSTREAM_IDS, 5] and {int(h["issue_src_glob_id"]) for h, _ in parts} == {0xAB00000001}
    assert wire.resol_messages(rows[:0]) == (b"", 0)
