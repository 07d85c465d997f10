"""the kernel sources carry no compile-time A/B switches beyond the listed ones: an experiment lives as a patch plus its numbers under
profiles/ (EXPERIMENTS.md, "Retired compile-time variants"), not as a second form behind an #if in the default source"""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# GYS_* names a conditional directive under gyeeta_amd/csrc/ may test
INSTRUMENTATION = {"GYS_RESP_TIMING", "GYS_HUGE_TIMING", "GYS_RESP_DBG", "GYS_MB_SKIP", "GYS_CONN_SKIP"}
SIZING = {"GYS_MB_WAVES16", "GYS_CONN_THREADS", "GYS_CONN_SPAN", "GYS_CONN_AGG_BITS", "GYS_CONN_HQ", "GYS_HB_CHUNK", "GYS_HB_WAVES",
          "GYS_RB_NT", "GYS_RB_AHEAD", "GYS_RB_WAVES", "GYS_RB_VC"}
KEMU_HOOKS = {"GYS_OPAQUE_VGPR", "GYS_OPAQUE_LOADED4", "GYS_DYN_LDS"}  # tests/cpp/kemu defines them its own way
OPEN_FINDING = {"GYS_PARK_INDEX"}  # both arms stay until the fix of its LDS pointer arithmetic
# rejected variants whose removal changes the device code of the default build (EXPERIMENTS.md names the kernels): they leave with
# the next change of those kernels
HELD_BACK = {"GYS_EV_DMA", "GYS_EV_DMA_AHEAD", "GYS_EV_DMA_CPOL", "GYS_MB_GROUP"}
ALLOWED = INSTRUMENTATION | SIZING | KEMU_HOOKS | OPEN_FINDING | HELD_BACK

RETIRED = ["GYS_BUCKET_LUT", "GYS_BK_BYTES", "GYS_SHIFT_SWITCH", "GYS_PROBE_XOR", "GYS_PROBE_JOINT", "GYS_EV_PREFETCH", "GYS_EV_NT",
           "GYS_EV_LOAD", "GYS_EV_SADDR", "GYS_EV_X3", "GYS_FLOOR_QUARTER", "GYS_HASH_FLAT", "GYS_GH_PER_WAVE", "GYS_RESP_KERNARG",
           "GYS_MB_PACKED", "GYS_MB_KERNARG", "GYS_MB_FUSE_OLD", "GYS_MB_COMPACT", "GYS_CONN_PREFETCH", "GYS_CONN_FLOOR", "GYS_HB_PIPE",
           "GYS_HB_STAGED", "GYS_HB_LUT", "GYS_KERNARG"]

# run-time switches (getenv) that selected a variant the project's own tables rejected, or an A/B leg (EXPERIMENTS.md, "Retired run-time
# switches"); the old round scripts under tools/ name them: those are records and are not scanned for these names
RETIRED_RUNTIME = ["GYS_OLD_MERGE", "GYS_CLASS1_GENERAL", "GYS_CLASS2_HUGE", "GYS_OLD_HUGE", "GYS_TPT", "GYS_TBL_SPARSE", "GYS_RQ_ONE_STREAM",
                   "GYS_NO_RESP_QUEUE", "GYS_NO_PRESPILL"]


def _hits(names, files):
    pat = re.compile(r"\b(" + "|".join(names) + r")\b")
    hits = []
    for path in files:
        if not os.path.isfile(path) or os.path.abspath(path) == os.path.abspath(__file__):
            continue
        if path.endswith((".so", ".pyc", ".o")) or os.sep + "golden" + os.sep in path:
            continue
        for no, line in enumerate(open(path, errors="replace"), 1):
            if pat.search(line):
                hits.append("%s:%d" % (os.path.relpath(path, ROOT), no))
    return hits


def test_conditional_directives_name_listed_switches_only():
    seen = set()
    for path in glob.glob(os.path.join(ROOT, "gyeeta_amd", "csrc", "*")):
        for line in open(path, errors="replace"):
            if re.match(r"\s*#\s*(if|ifdef|ifndef|elif)\b", line):
                seen.update(re.findall(r"\bGYS_[A-Za-z0-9_]+", line.split("//")[0]))
    assert seen, "no conditional directive found: wrong directory?"
    assert not sorted(seen - ALLOWED), sorted(seen - ALLOWED)


def test_retired_switches_are_gone():
    files = [p for d in ("gyeeta_amd", "include", "tests") for p in glob.glob(os.path.join(ROOT, d, "**", "*"), recursive=True)]
    assert len(files) > 50
    hits = _hits(RETIRED, files + glob.glob(os.path.join(ROOT, "tools", "*.sh"))) + _hits(RETIRED_RUNTIME, files)
    assert not hits, hits
