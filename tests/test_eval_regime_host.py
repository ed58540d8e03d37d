"""CPU tests (-m "not gpu") of the eval forward's regime gauge (csrc/forward_eval.hip yolat_eval_regime_*) and of the graph
preparation plan per regime (csrc/graph.hip, yolat_graph_prepare_plan_regime).

The gauge is driven through yolat_eval_regime_observe with synthetic stream keys and clocks: a forward takes the
throughput regime when at least K = 3 distinct streams enqueued a forward within the last W = 1 ms, its own included.
The table is process-global, so every test moves to a clock range of its own, far past everything recorded before it.
The plan is checked through its contract (include/yolat_hip.h), not a restatement of the rule."""
import ctypes
import os
import subprocess
import sys

import pytest

from yolat_vectorgraphicsrecognition_amd import _lib

pytestmark = pytest.mark.host

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K, W_NS, SLOTS = 3, 1_000_000, 64
LATENCY, THROUGHPUT = 0, 1
lib = _lib.lib

_epoch = [0]


def fresh_clock():
    """a start time no earlier test's records can reach: one second past the previous one"""
    _epoch[0] += 1_000_000_000
    return _epoch[0]


def observe(stream, now):
    return lib.yolat_eval_regime_observe(stream, now)


@pytest.fixture(autouse=True)
def auto_mode():
    assert lib.yolat_eval_regime_set(0) == 0
    yield
    assert lib.yolat_eval_regime_set(0) == 0


def test_one_stream_back_to_back_stays_in_the_latency_regime():
    t = fresh_clock()
    for i in range(500):
        assert observe(0xA0, t + 50 * i) == LATENCY              # 20 forwards per microsecond-scale step: still one stream


def test_k_distinct_streams_inside_the_window_switch_on_the_kth_call():
    t = fresh_clock()
    got = [observe(0xB0 + i, t + 10_000 * i) for i in range(K + 2)]
    assert got == [LATENCY] * (K - 1) + [THROUGHPUT] * 3
    assert observe(0xB0, t + 10_000 * (K + 2)) == THROUGHPUT     # a stream already counted stays counted


def test_the_same_streams_spread_wider_than_the_window_stay_in_the_latency_regime():
    t = fresh_clock()
    for i in range(4 * K):
        assert observe(0xC0 + i % K, t + (W_NS // (K - 1) + 1) * i) == LATENCY    # never K of them inside one window


def test_the_regime_falls_back_once_the_window_has_passed():
    t = fresh_clock()
    for i in range(K):
        last = observe(0xD0 + i, t + 1000 * i)
    assert last == THROUGHPUT
    assert observe(0xD0, t + 1000 * (K - 1) + W_NS // 2) == THROUGHPUT
    assert observe(0xD0, t + 1000 * (K - 1) + 2 * W_NS) == LATENCY
    assert observe(0xD0, t + 1000 * (K - 1) + 2 * W_NS + 10) == LATENCY


def test_more_streams_than_table_slots_still_report_throughput():
    t = fresh_clock()
    got = [observe(0x10000 + i, t + 100 * i) for i in range(4 * SLOTS)]
    assert got[:K - 1] == [LATENCY] * (K - 1) and all(r == THROUGHPUT for r in got[K - 1:])
    # the evicted streams are the oldest: the most recent ones are still in the table and inside the window
    assert observe(0x10000 + 4 * SLOTS - 1, t + 100 * 4 * SLOTS) == THROUGHPUT


def test_set_and_get():
    t = fresh_clock()
    assert lib.yolat_eval_regime_get() == 0
    assert lib.yolat_eval_regime_set(2) == 0 and lib.yolat_eval_regime_get() == 2
    assert observe(0xE0, t) == THROUGHPUT                        # forced: one stream is enough
    assert lib.yolat_eval_regime_set(1) == 0 and lib.yolat_eval_regime_get() == 1
    assert [observe(0xE0 + i, t + 10 + i) for i in range(2 * K)] == [LATENCY] * (2 * K)
    assert lib.yolat_eval_regime_set(0) == 0
    assert observe(0xE0, t + 100) == THROUGHPUT                  # forced modes still record: auto sees those streams
    for bad in (-1, 3):
        assert lib.yolat_eval_regime_set(bad) == -1 and lib.yolat_eval_regime_get() == 0


def test_counts_report_forwards_not_observations():
    out = (ctypes.c_int64 * 2)(-1, -1)
    assert lib.yolat_eval_regime_counts(out) == 0
    before = list(out)
    observe(0xF0, fresh_clock())
    assert lib.yolat_eval_regime_counts(out) == 0 and list(out) == before and min(before) >= 0
    assert lib.yolat_eval_regime_counts(None) == -1


def test_environment_switches_are_read_once_and_the_setter_wins():
    script = ("import sys\n"
              "sys.path.insert(0, %r)\n"
              "from yolat_vectorgraphicsrecognition_amd import _lib\n"
              "lib = _lib.lib\n"
              "out = [lib.yolat_eval_regime_get()]\n"
              "out.append([lib.yolat_eval_regime_observe(7 + i, 1000 + i) for i in range(4)])\n"
              "lib.yolat_eval_regime_set(1)\n"
              "out.append(lib.yolat_eval_regime_get())\n"
              "out.append(lib.yolat_eval_regime_observe(99, 2000))\n"
              "lib.yolat_eval_regime_set(0)\n"
              "out.append([lib.yolat_eval_regime_observe(200 + i, 10**10 + 400000 * i) for i in range(4)])\n"
              "print(out)\n" % REPO)

    def child(**env):
        base = {k: v for k, v in os.environ.items() if not k.startswith("YOLAT_EVAL_REGIME")}
        r = subprocess.run([sys.executable, "-c", script], env=dict(base, **env), capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        return eval(r.stdout.strip().splitlines()[-1])

    spread = [0, 0, 1, 1]          # 0.4 ms apart: three inside 1 ms from the third call on
    assert child() == [0, [0, 0, 1, 1], 1, 0, spread]
    assert child(YOLAT_EVAL_REGIME="auto") == [0, [0, 0, 1, 1], 1, 0, spread]
    assert child(YOLAT_EVAL_REGIME="latency") == [1, [0, 0, 0, 0], 1, 0, spread]
    assert child(YOLAT_EVAL_REGIME="throughput") == [2, [1, 1, 1, 1], 1, 0, spread]
    assert child(YOLAT_EVAL_REGIME="bogus") == [0, [0, 0, 1, 1], 1, 0, spread]
    # the measurement switches: K = 2 streams; a 500 us window holds only two of the calls 400 us apart
    assert child(YOLAT_EVAL_REGIME_STREAMS="2") == [0, [0, 1, 1, 1], 1, 0, [0, 1, 1, 1]]
    assert child(YOLAT_EVAL_REGIME_WINDOW_US="500") == [0, [0, 0, 1, 1], 1, 0, [0, 0, 0, 0]]


# ---------------------------------------------------------------------------------------------
# the graph-preparation plan per regime
# ---------------------------------------------------------------------------------------------
PS_RMAX, PS_CAP, GRID_MAX = 256, 4096, 250
SWEEP_N = [1, 2, 15, 16, 33, 255, 256, 257, 300, 1000, 4097, 9999, 10000, 10240, 20000, 28000, 43520, 45000, 63999, 64000,
           64001, 70000, 200000]
SWEEP_E = [0, 1, 7, 2047, 2048, 2049, 4096, 20000, 40000, 52976, 90001, 98303, 98304, 98305, 140001, 1200000]


def plan(N, E, other):
    rows, wgs = ctypes.c_int32(-1), ctypes.c_int32(-1)
    form = lib.yolat_graph_prepare_plan(N, E, other, ctypes.byref(rows), ctypes.byref(wgs))
    return form, rows.value, wgs.value


def plan_regime(N, E, other, regime):
    rows, wgs = ctypes.c_int32(-1), ctypes.c_int32(-1)
    form = lib.yolat_graph_prepare_plan_regime(N, E, other, regime, ctypes.byref(rows), ctypes.byref(wgs))
    return form, rows.value, wgs.value


def riders(N):
    return -(-(N + 1) // 1024) + -(-N // 256)


def cdiv(a, b):
    return -(-a // b)


@pytest.mark.parametrize("with_riders", [False, True])
def test_latency_plan_is_the_plain_plan_over_the_sweep(with_riders):
    for N in SWEEP_N:
        for E in SWEEP_E:
            other = riders(N) if with_riders else 0
            assert plan_regime(N, E, other, LATENCY) == plan(N, E, other), (N, E, other)


def test_throughput_plan_of_the_headline():
    assert plan_regime(10000, 40000, riders(10000), THROUGHPUT) == (1, 250, 40)      # a 90-workgroup launch
    assert riders(10000) == 50
    assert plan_regime(10000, 40000, riders(10000), LATENCY) == (1, 100, 100)
    assert plan_regime(10000, 40000, 50, 2) == (0, 0, 0) and plan_regime(10000, 40000, 50, -1) == (0, 0, 0)
    lib.yolat_graph_prepare_plan_regime(10000, 40000, 50, THROUGHPUT, None, None)     # NULL outputs are allowed


@pytest.mark.parametrize("with_riders", [False, True])
def test_throughput_plan_invariants_over_the_sweep(with_riders):
    seen = {0: 0, 1: 0}
    fatter = 0
    for N in SWEEP_N:
        for E in SWEEP_E:
            other = riders(N) if with_riders else 0
            form, R, wgs = plan_regime(N, E, other, THROUGHPUT)
            lat = plan(N, E, other)
            seen[form] += 1
            assert form == lat[0], (N, E, other)                  # one launch exactly where the latency plan takes it
            if not form:
                assert R == 0 and wgs == 0
                continue
            assert 1 <= R <= PS_RMAX, (N, E, R)
            assert wgs == cdiv(N, R), (N, E, R, wgs)
            assert wgs + other <= GRID_MAX, (N, E, R, wgs, other)
            assert R == 1 or R * E <= (PS_CAP // 2) * N, (N, E, R)
            assert R >= lat[1], (N, E, R, lat)                    # never more workgroups than one at a time
            fatter += R > lat[1]
    assert seen[0] > 0 and seen[1] > 0 and fatter > 0


def test_forced_rows_override_both_regimes():
    script = ("import ctypes, sys\n"
              "sys.path.insert(0, %r)\n"
              "from yolat_vectorgraphicsrecognition_amd import _lib\n"
              "out = []\n"
              "for regime in (0, 1):\n"
              "    r, w = ctypes.c_int32(), ctypes.c_int32()\n"
              "    f = _lib.lib.yolat_graph_prepare_plan_regime(10000, 40000, 50, regime, ctypes.byref(r), ctypes.byref(w))\n"
              "    out.append((f, r.value, w.value))\n"
              "print(out)\n" % REPO)

    def child(**env):
        r = subprocess.run([sys.executable, "-c", script], env=dict(os.environ, **env), capture_output=True, text=True,
                           timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        return eval(r.stdout.strip().splitlines()[-1])

    assert child(YOLAT_PREP_R="50") == [(1, 50, 200)] * 2
    assert child(YOLAT_PREP_SMALL="0") == [(0, 0, 0)] * 2
