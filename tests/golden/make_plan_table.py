"""Generate tests/golden/plan_table.json -- what bicos_match_plan answers over a table of
shapes and configurations.

bicos_match_plan (include/bicos_c.h) makes no HIP call and accepts a NULL engine, which
plans as a 256-CU device does. The table pins its answers, the BICOS_PLAN_* bits or a
negative error code, so that a change to the host orchestration can be shown to plan every
match as before: tests/test_plan_table.py compares the library with the file entry for
entry, on the CPU with a NULL engine and on the GPU with a real, untuned one.

The table is the product of AXES, in the order of `cases()`, and then EXTRA:
  * (mode, n): both sides of every descriptor word count, one-pass and fusion boundary;
    LIMITED 66 and FULL 17 need more than 256 bits (BICOS_E_BITS)
  * cols / rows / depth, a row pitch of cols and of cols rounded up to 4, stack bases 0
    and 2 (the LDS-staged agree needs dword-aligned stacks)
  * NoDuplicates, Consistency, Consistency with no_dupes; with and without the NXC stage,
    a subpixel step, DOUBLE precision
  * EXTRA: n = 1 and depth 3 (BICOS_E_ARG)

Run it at the commit whose plans are the yardstick; it is independent of the environment
only while no BICOS_* switch is set.

  python tests/golden/make_plan_table.py [--lib path/to/libbicos_amd.so]
"""
import ctypes
import itertools
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from libbicos_amd import _lib  # noqa: E402

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "plan_table.json")

AXES = {
    "mode_n": [(0, n) for n in (2, 3, 4, 8, 9, 10, 17, 18, 33, 34, 40, 41, 65, 66)] +
              [(1, n) for n in (6, 8, 12, 13, 16, 17)],
    "cols": [1, 640, 1023, 1024, 2048, 2049, 3208, 8160, 8161],
    "rows": [1, 480],
    "depth": [1, 2],
    "pitch4": [0, 1],          # row pitch: cols | cols rounded up to 4
    "base": [0, 2],            # address of both stacks
    "variant": [(0, 0), (1, 0), (1, 1)],   # (variant_type, no_dupes)
    "nxcorr": [0, 1],
    "step": [-1.0, 0.1],
    "precision": [0, 1],
}
# (mode, n, cols, rows, depth): argument errors, planned like any other row
EXTRA = [(0, 1, 640, 480, 1), (0, 8, 640, 480, 3), (1, 1, 640, 480, 1), (0, 33, 2048, 480, 0)]


def cases():
    """Every row of the table as the arguments of plan_of, in file order."""
    for (mode, n), cols, rows, depth, p4, base, (vt, nd), nx, step, prec in \
            itertools.product(*AXES.values()):
        pitch = (cols + 3) // 4 * 4 if p4 else cols
        yield n, rows, cols, pitch, depth, base, (0.9, step, -1.0, mode, prec, vt, 1, nd), nx
    for mode, n, cols, rows, depth in EXTRA:
        yield n, rows, cols, cols, depth, 0, (0.9, -1.0, -1.0, mode, 0, 0, 1, 0), 1


def plan_of(L, engine, n, rows, cols, pitch, depth, base, cfg, has_nxcorr):
    c = _lib.BicosConfig(*cfg)
    return L.bicos_match_plan(engine, base, base, n, rows, cols, pitch, rows * pitch, depth,
                              ctypes.byref(c), has_nxcorr)


def table(L, engine=None):
    return [plan_of(L, engine, *case) for case in cases()]


def bind(path):
    """a library at another path (a build of another commit) with bicos_match_plan typed"""
    L = ctypes.CDLL(path)
    P, I, Z = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t
    L.bicos_match_plan.argtypes = [P, P, P, I, I, I, Z, Z, I, ctypes.POINTER(_lib.BicosConfig), I]
    L.bicos_match_plan.restype = I
    return L


def main(argv):
    L = bind(argv[argv.index("--lib") + 1]) if "--lib" in argv else _lib.lib()
    plans = table(L)
    axes = {k: [list(v) if isinstance(v, tuple) else v for v in vs] for k, vs in AXES.items()}
    with open(PATH, "w") as f:
        json.dump({"axes": axes, "extra": [list(e) for e in EXTRA], "plans": plans}, f,
                  separators=(",", ":"))
        f.write("\n")
    print("wrote %s: %d rows, %d distinct answers" % (PATH, len(plans), len(set(plans))))


if __name__ == "__main__":
    main(sys.argv[1:])
