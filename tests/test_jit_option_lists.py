"""The hiprtc option lists of the run-time builds (not gpu).  A list decides which kernel is compiled and is the text of the disk
cache's key, so it must not move when the code that spells it is rearranged: tests/golden/jit_option_lists.json holds the lists of the
matrix below as the commit BEFORE the build spec (RsJitSpec, csrc/rs_host.h) produced them -- recorded from that commit's positional
rs_jit_options behind the same export -- and rs_jit_option_text must return them string for string, in the same order.

Recording (only ever from a library whose lists are known to be right):
    python tests/test_jit_option_lists.py <library with rs_jit_option_text> > tests/golden/jit_option_lists.json

The second test keeps the host-only build of tools/sanitize_cpu.sh linkable: the launcher stubs must define every launcher that
rs_api.cpp calls, with the signatures of rs_host.h."""
import ctypes as C
import json
import os
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
GOLDEN_FILE = ROOT / "tests" / "golden" / "jit_option_lists.json"

SCHEDS = (1, 7, 8, 9, 10, 11, 101, 103)
# S, U, R, G, NT: the headline grid (one sort position per lane), the 64-RBG grid at 640 and at 1 024 threads (two positions per lane,
# RS_JIT_WPE follows the carve) and at 512 (three)
A, B, C_, D = (20, 500, 25, 4, 512), (20, 500, 64, 8, 640), (20, 500, 64, 8, 1024), (20, 100, 64, 8, 512)
# RsGroupForm::jit_flags, every row of the table (the counted run's too: the option list knows nothing of the refusal)
FORM_FLAGS = (8, 8 | 16, 8 | 32, 8 | 128, 8 | 32 | 64, 8 | 16 | 256, 8 | 16 | 64 | 256)
VARIANTS = (None, "-DRS_JIT_RECORDS=1", "-DRS_JIT_CELL_CONFIGS=6", "ss=default -DX=1", "ss=iterative-ilp")
ENVS = ({"RS_JIT_EXTRA": "-DX=1  -DY=2"}, {"RS_JIT_SCHED_STRATEGY": "default"}, {"RS_JIT_SCHED_STRATEGY": "max-ilp"},
        {"RS_JIT_EXTRA": "-DRS_JIT_RECORDS=1", "RS_JIT_SCHED_STRATEGY": "max-occupancy"})


def matrix():
    """Every branch of rs_jit_options both ways; a row is the export's arguments and the environment of the call."""
    rows = []

    def add(shape, sched, qmode=0, win=0, flags=0, variant=None, tuned=1, env=None):
        rows.append({"shape": list(shape), "sched": sched, "qmode": qmode, "win": win, "flags": flags, "variant": variant, "tuned": tuned,
                     "env": env or {}})

    for sched in SCHEDS:
        shapes = (A,) + ((B,) if sched in (8, 9, 10, 101) else ()) + ((C_,) if sched in (9, 10, 11) else ()) + ((D,) if sched == 9 else ())
        for shape in shapes:
            for win in (0, 8, 32, 40):                      # batches: the slice window
                add(shape, sched, win=win)
            for win in (0, 40):
                add(shape, sched, win=win, tuned=0)
                for flags in (2, 4, 6):                     # ... streamed, lean, both
                    add(shape, sched, win=win, flags=flags)
            for qmode, flags in ((2, 0), (2, 4), (3, 0)):   # ... with the queue model
                add(shape, sched, qmode=qmode, flags=flags)
            add(shape, sched, qmode=2, win=40, flags=2, tuned=0)
            for flags, tuned in ((1, 0), (1, 1), (1 | 4, 1)):  # drop-in contexts, with and without the gate scratch
                add(shape, sched, qmode=1, flags=flags, tuned=tuned)
            add(shape, sched, qmode=0, flags=1)
    for form in FORM_FLAGS:                                 # group builds
        for lean in (0, 4):
            for shape, sched, qmode in ((A, 1, 1), (A, 9, 0), (B, 9, 0)):
                add(shape, sched, qmode=qmode, flags=form | lean)
            add(A, 8, flags=1 | form | lean, tuned=0)
    for variant in VARIANTS:                                # autotune candidates and the batch kernel's compile-time switches
        for sched in (8, 9, 11):
            for flags, tuned in ((0, 0), (0, 1), (4, 1)):
                add(A, sched, win=32, flags=flags, variant=variant, tuned=tuned)
        add(B, 9, qmode=2, variant=variant)
    for env in ENVS:                                        # the tuning variables of the environment
        for sched in (1, 8, 9):
            for variant in (None, "ss=default -DX=1", "-DRS_JIT_RECORDS=1 -DRS_JIT_CELL_CONFIGS=1"):
                add(A, sched, win=8, variant=variant, env=env)
            add(A, sched, win=8, tuned=0, env=env)
    return rows


def option_list(L, row):
    """rs_jit_option_text for one row, with the row's environment set for the call and restored after it."""
    fn = L.rs_jit_option_text
    fn.restype = C.c_int
    fn.argtypes = [C.c_int] * 9 + [C.c_char_p, C.c_int, C.c_char_p, C.c_size_t]
    names = ("RS_JIT_EXTRA", "RS_JIT_SCHED_STRATEGY")
    saved = {k: os.environ.get(k) for k in names}
    try:
        for k in names:
            os.environ.pop(k, None)
        os.environ.update(row["env"])
        buf = C.create_string_buffer(8192)
        variant = None if row["variant"] is None else row["variant"].encode()
        n = fn(*row["shape"], row["sched"], row["qmode"], row["win"], row["flags"], variant, row["tuned"], buf, len(buf))
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v
    assert 0 < n < len(buf) and len(buf.value) == n
    return buf.value.decode().split("\n")


def test_option_lists_are_the_recorded_ones(rs):
    golden = json.loads(GOLDEN_FILE.read_text())
    rows = matrix()
    assert [{k: g[k] for k in g if k != "options"} for g in golden] == rows, "the golden file was recorded for another matrix"
    L = rs.lib()
    assert hasattr(L, "rs_jit_option_text")
    for g in golden:
        assert option_list(L, g) == g["options"], {k: g[k] for k in g if k != "options"}
    # the matrix reaches what it is there for: every optional spelling appears in some list and is absent from another
    seen = {o.split("=")[0] for g in golden for o in g["options"]}
    for opt in ("-DRS_P3_BLOCK_TOP", "-DRS_JIT_STREAMED", "-DRS_JIT_LEAN", "-DRS_JIT_GROUP", "-DRS_JIT_GROUP_RESIDENT", "-DRS_JIT_GROUP_QUEUED",
                "-DRS_JIT_GROUP_COUNTED", "-DRS_JIT_GROUP_FLOWS", "-DRS_JIT_GROUP_RUN", "-fno-slp-vectorize", "-mllvm", "-amdgpu-sched-strategy",
                "-DRS_JIT_CELL_CONFIGS", "-DX", "-DY"):
        assert opt in seen, opt
        assert any(all(o.split("=")[0] != opt for o in g["options"]) for g in golden), opt
    for value in ("-DRS_P3_BLOCK=8", "-DRS_P3_BLOCK=16", "-DRS_P3_BLOCK=32", "-DRS_JIT_RECORDS=0", "-DRS_JIT_RECORDS=1", "-DRS_JIT_WPE=4", "-DRS_JIT_WPE=5",
                  "-DRS_JIT_WPE=8", "-amdgpu-sched-strategy=iterative-ilp", "-amdgpu-sched-strategy=max-ilp"):
        assert any(value in g["options"] for g in golden), value


def test_host_only_build_links_against_the_launcher_stubs(tmp_path):
    from radiosaber_amd import build
    build.write_tables_inc()
    build.write_link_pinned_inc()
    build.write_jit_sources()
    cmd = ["g++", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-Iinclude",
           "radiosaber_amd/csrc/rs_api.cpp", "radiosaber_amd/csrc/rs_jit.cpp", "tests/csrc/host_launch_stubs.cpp",
           "-L/opt/rocm/lib", "-lamdhip64", "-lhiprtc", "-Wl,--no-undefined", "-o", str(tmp_path / "libradiosaber_hip_host.so")]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]


if __name__ == "__main__":
    lib = C.CDLL(sys.argv[1])
    print("[\n" + ",\n".join(json.dumps(dict(row, options=option_list(lib, row)), separators=(",", ":")) for row in matrix()) + "\n]")
