"""CPU tests (-m "not gpu") of the launch planner of yolat_graph_prepare (csrc/graph.hip prep_small_rows), through the
library's own query yolat_graph_prepare_plan — the rule is not restated here, only its contract (include/yolat_hip.h):
the one-launch form (k_prep_small) needs E <= 98304, rows per workgroup <= 256, rows * E / N <= 2048 (half the 4096 list
slots at uniform degree; one row is the floor) and a grid of at most 250 workgroups with the riding segment / node-side
workgroups; the four-launch form is taken exactly where no plan meets that."""
import ctypes
import os
import subprocess
import sys

import pytest

from yolat_vectorgraphicsrecognition_amd import _lib

PS_RMAX, PS_CAP, E_MAX, GRID_MAX = 256, 4096, 98304, 250
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def plan(N, E, other):
    rows, wgs = ctypes.c_int32(-1), ctypes.c_int32(-1)
    form = _lib.lib.yolat_graph_prepare_plan(N, E, other, ctypes.byref(rows), ctypes.byref(wgs))
    return form, rows.value, wgs.value


def riders(N):
    """the workgroups that ride in the launch in a forward: proposal segments + node side of the first conv layer"""
    return -(-(N + 1) // 1024) + -(-N // 256)


def cdiv(a, b):
    return -(-a // b)


CFG = {"cfg1": (43520, 52976), "cfg2": (10000, 40000), "cfg5": (200000, 1200000)}
SWEEP_N = [1, 2, 15, 16, 33, 255, 256, 257, 300, 1000, 4097, 9999, 10000, 10240, 20000, 28000, 43520, 45000, 63999, 64000,
           64001, 70000, 200000]
SWEEP_E = [0, 1, 7, 2047, 2048, 2049, 4096, 20000, 40000, 52976, 90001, 98303, 98304, 98305, 140001, 1200000]


@pytest.mark.parametrize("with_riders", [False, True])
def test_plan_invariants_over_a_sweep(with_riders):
    seen = {0: 0, 1: 0}
    for N in SWEEP_N:
        for E in SWEEP_E:
            other = riders(N) if with_riders else 0
            form, R, wgs = plan(N, E, other)
            seen[form] += 1
            # the one-launch form exactly where the limits leave a plan: the most workgroups the round has room for
            # give the smallest R, so if that R breaks a limit every plan does
            room = GRID_MAX - other
            r_edges = max(1, (PS_CAP // 2) * N // E) if E > 0 else PS_RMAX
            feasible = E <= E_MAX and room >= 1 and cdiv(N, room) <= min(PS_RMAX, r_edges)
            assert form == (1 if feasible else 0), (N, E, other, form, R, wgs)
            if not form:
                assert R == 0 and wgs == 0
                continue
            assert 1 <= R <= PS_RMAX, (N, E, R)
            assert wgs == cdiv(N, R) and wgs * R >= N, (N, E, R, wgs)
            assert wgs + other <= GRID_MAX, (N, E, R, wgs, other)
            # uniform degree: a workgroup's R rows hold R * E / N edges — at most half the list (R = 1 cannot go lower)
            assert R == 1 or R * E <= (PS_CAP // 2) * N, (N, E, R)
    assert seen[0] > 0 and seen[1] > 0


def test_plan_of_the_benchmark_configs():
    # cfg 2 (the headline): 100 CSR workgroups of 100 rows, 400 edges each, in a 150-workgroup launch
    assert plan(*CFG["cfg2"], riders(CFG["cfg2"][0])) == (1, 100, 100)
    assert plan(*CFG["cfg2"], 0) == (1, 100, 100)                # ops.build_graph: no riders
    # cfg 1: 213 riding workgroups leave 37 of the round, 1177 rows each -> four launches in a forward
    assert plan(*CFG["cfg1"], riders(CFG["cfg1"][0])) == (0, 0, 0)
    assert plan(*CFG["cfg1"], 0) == (1, 175, 249)                # alone it fits one round, with fatter workgroups
    # cfg 5: above the E limit either way
    assert plan(*CFG["cfg5"], riders(CFG["cfg5"][0])) == (0, 0, 0)
    assert plan(*CFG["cfg5"], 0) == (0, 0, 0)


def test_plan_limits():
    assert plan(20000, 98304, 0) == (1, 100, 200)
    assert plan(20000, 98305, 0) == (0, 0, 0)
    assert plan(64000, 1000, 0) == (1, 256, 250)
    assert plan(64001, 1000, 0) == (0, 0, 0)                      # 251 workgroups of 256 rows
    assert plan(64000, 1000, 1) == (0, 0, 0)
    assert plan(25000, 98304, riders(25000)) == (1, 197, 127)     # the round's room decides, within both limits
    assert plan(300, 20000, 0) == (1, 30, 10)                     # the edge headroom decides: 30 rows hold 2000 edges
    assert plan(0, 10, 0) == (0, 0, 0) and plan(10, -1, 0) == (0, 0, 0) and plan(10, 10, 250) == (0, 0, 0)
    assert plan(11, 500, 0) == (1, 11, 1)                         # N < R: one workgroup
    assert plan(3, 20000, 0) == (1, 1, 3)                         # degree > 2048: one row per workgroup is the floor
    _lib.lib.yolat_graph_prepare_plan(10000, 40000, 50, None, None)        # NULL outputs are allowed


def test_plan_switches_are_read_once_per_process():
    """YOLAT_PREP_R forces the rows per workgroup (any grid) within the E limit; values outside 1..256 are ignored;
    YOLAT_PREP_SMALL=0 turns the one-launch form off.  Both are read once per process, hence child processes."""
    script = ("import ctypes, sys\n"
              "sys.path.insert(0, %r)\n"
              "from yolat_vectorgraphicsrecognition_amd import _lib\n"
              "out = []\n"
              "for N, E, o in ((10000, 40000, 50), (43520, 52976, 213), (200000, 1200000, 978), (11, 500, 0)):\n"
              "    r, w = ctypes.c_int32(), ctypes.c_int32()\n"
              "    f = _lib.lib.yolat_graph_prepare_plan(N, E, o, ctypes.byref(r), ctypes.byref(w))\n"
              "    out.append((f, r.value, w.value))\n"
              "print(out)\n" % REPO)

    def child(**env):
        r = subprocess.run([sys.executable, "-c", script], env=dict(os.environ, **env), capture_output=True, text=True,
                           timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        return eval(r.stdout.strip().splitlines()[-1])

    assert child(YOLAT_PREP_R="50") == [(1, 50, 200), (1, 50, 871), (0, 0, 0), (1, 50, 1)]
    assert child(YOLAT_PREP_R="256") == [(1, 256, 40), (1, 256, 170), (0, 0, 0), (1, 256, 1)]
    assert child(YOLAT_PREP_R="257") == [(1, 100, 100), (0, 0, 0), (0, 0, 0), (1, 11, 1)]
    assert child(YOLAT_PREP_R="0") == [(1, 100, 100), (0, 0, 0), (0, 0, 0), (1, 11, 1)]
    assert child(YOLAT_PREP_SMALL="0") == [(0, 0, 0)] * 4
    assert child(YOLAT_PREP_SMALL="0", YOLAT_PREP_R="50") == [(0, 0, 0)] * 4
