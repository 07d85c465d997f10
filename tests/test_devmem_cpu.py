"""Who owns device and pinned memory, without a GPU.

Structure: gyeeta_amd/csrc/gys_devmem.hpp (DevBuf, PinnedPair) is the only file of the library that calls the HIP allocation entry points,
gys_destroy keeps no hand-written free list, and no member of gys_ctx is a raw pointer except the views listed here -- a new raw owner
fails the test.

Behaviour: tests/cpp/test_devmem.cc, a stand-alone program (its own main) compiled by g++ with AddressSanitizer and UBSan over the CPU
stand-in of the HIP header (tests/cpp/kemu, as tests/test_resp_plan_cpu.py) and a fake allocator that counts live blocks and can fail the
k-th allocation: grow / alloc / the contents-keeping grow, what a failed allocation leaves behind, swap and move, the seven arrays of the
wire front end's reservation.  Nothing is loaded into Python."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gyeeta_amd", "csrc")
KEMU = os.path.join(ROOT, "tests", "cpp", "kemu")
ALLOC_CALLS = ("hipMalloc(", "hipFree(", "hipHostMalloc(", "hipHostFree(")

# gys_ctx members that may be declared `= nullptr`: VIEWS and runtime handles, none of which owns memory
RAW_POINTER_VIEWS = {("uint8_t", "arena"),  # the caller's reduce arena, or arena_own
                     ("std::mutex", "enq_mu")}  # IngestEnv: the context's own enqueue mutex
HANDLE_TYPES = {"hipStream_t", "hipGraph_t", "hipGraphExec_t", "hipEvent_t"}  # destroyed explicitly, in order, by gys_destroy
HANDLES = {("hipStream_t", "stream"), ("hipStream_t", "copy_stream"), ("hipGraph_t", "win_graph"), ("hipGraphExec_t", "win_graph_exec"),
           ("hipGraph_t", "g"), ("hipGraphExec_t", "x"), ("hipEvent_t", "done"), ("hipEvent_t", "copied")}


def _src(name):
    return open(os.path.join(CSRC, name)).read()


def test_only_devmem_calls_the_allocator():
    users = {f for f in sorted(os.listdir(CSRC)) if any(c in _src(f) for c in ALLOC_CALLS)}
    assert users == {"gys_devmem.hpp"}, users
    assert "gys_devmem.hpp" in __import__("gyeeta_amd.build", fromlist=["DEPS"]).DEPS


def test_destroy_has_no_free_list():
    assert "ptrs[]" not in _src("gys_engine.hip")


# the structs of gys_subq.hpp that gys_ctx holds by value (the submission queues, the staging ring, what both use of the context): their
# members are members of the context
SUBQ_STRUCTS = ("SubQ", "IngestEnv", "Stage", "StageRing")


def _struct_body(s, head):
    a = s.index(head)
    b = s.index("\n};\n", a)  # (the struct's own closing brace is the first one in column 0)
    body = re.sub(r"//[^\n]*", "", s[a + len(head):b])
    return re.sub(r"/\*.*?\*/", "", body, flags=re.S)


def _ctx_body():
    body = _struct_body(_src("gys_engine.hip"), "struct gys_ctx {")
    for name in SUBQ_STRUCTS:
        assert re.search(r"\b%s \w+(\[\w*\])?;" % name, body) or name == "Stage", name  # (Stage: inside StageRing)
        body += ";" + _struct_body(_src("gys_subq.hpp"), "struct %s {" % name)
    return body


def test_ctx_members_are_owners_or_listed_views():
    body = _ctx_body()
    assert "DevBuf<" in body and "PinnedPair<" in body
    raw, handles = set(), set()
    for stmt in body.split(";"):
        stmt = re.split(r"\{\s*\n", stmt)[-1]  # (the first member of a nested struct: drop the struct's head)
        names = re.findall(r"(\*?)\s*(\w+)(?:\[\w*\])?\s*(?:=\s*\{?\s*nullptr|\{\s*(?:nullptr)?\s*\})", stmt)
        # every pointer declarator, initialised or not (functions returning `const char *` are the one other use of '*')
        names += [("*", n) for n in re.findall(r"\*\s*(\w+)\s*(?:\[\w*\]\s*)?(?:=|,|$)", stmt.strip())]
        if not names:
            continue
        typ = re.match(r"\s*(?:static\s+|const\s+)*((?:unsigned long long)|[\w:]+)", stmt).group(1)
        for star, name in names:
            if star:
                raw.add((typ, name))
            elif typ in HANDLE_TYPES:
                handles.add((typ, name))
    assert raw == RAW_POINTER_VIEWS, raw
    assert handles == HANDLES, handles
    assert len(re.findall(r"const char \*", body)) == 1 and "const char *word() const" in body  # (a function: error texts)


@pytest.fixture(scope="module")
def devmem_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("devmem") / "test_devmem")
    p = subprocess.run(["g++", "-std=c++20", "-O1", "-g", "-w", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I" + KEMU,
                        os.path.join(ROOT, "tests", "cpp", "test_devmem.cc"), "-o", exe, "-pthread"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout[-3000:]
    return exe


def test_owners_under_a_failing_allocator(devmem_exe):
    p = subprocess.run(["timeout", "-s", "KILL", "120", devmem_exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert p.returncode == 0 and "devmem ok" in p.stdout and not p.stderr.strip(), (p.returncode, p.stdout[-2000:], p.stderr[-2000:])
