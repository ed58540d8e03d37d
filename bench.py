#!/usr/bin/env python
"""bench.py — throughput of the YOLaT GNN hot path on MI355X.

    python bench.py --gpus 1 --steps K --warmup W            # default: BASELINE.json configs[1]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
           --master-port P bench.py --gpus N --steps K --warmup W

A "step" is one pass of the hot path over one batch of synthetic input already resident in HBM:
  --mode fwd   (default)  SparseCADGCN eval forward of ONE synthetic Bezier graph per rank
                          (cfg 2: N=10 000 nodes / E=40 000 edges / P=400 proposals, in_channels=5,
                          n_blocks=2), including the device-side CSR / segment build from the raw COO
                          edge list.  Ranks are independent replicas on different graphs (seed+rank):
                          no data-path collective, weak scaling.
  --mode train            one training step (forward + CE + backward + Adam) of cfg 3/4 with ONE RCCL
                          all-reduce of the flat 6.45 MB gradient bucket per step when N > 1.
Rank 0 prints ONE JSON line.  `value` = graphs processed by all ranks / max-over-ranks wall time.

A plain run sets up, warms up, times the K steps and prints the line: `ms_per_step` = the timed wall time / K.
--full adds everything else the line can carry (one-forward latency, hand-over rates, rooflines, the CPU baseline, the
other configurations' sub-records); the --no-* switches trim that set.  --dump-outputs DIR writes what the last
timed step returned as DIR/<name>.npy (fwd: pred_cls, bbox; train: loss and every parameter after the step).
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REPO)

PEAK_MFMA_F32_TFLOPS = 157.3     # MI355X fp32-input MFMA dense peak (MI355X_MICROARCH.md)
PEAK_HBM_GBS = 8000.0            # HBM3E spec peak


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--mode", default="fwd", choices=["fwd", "train"])
    ap.add_argument("--config", default=None, help="cfg id 1..5 (default: 2 for fwd, 3 for train)")
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps, also measure everything beside the headline: latency, hand-over rates, "
                         "rooflines, CPU baseline, sub-records (minutes; a plain run does none of it)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step returned to DIR/<name>.npy (float32 / float64)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline")
    ap.add_argument("--no-roofline", action="store_true", help="with --full: skip the op tables and rooflines")
    ap.add_argument("--no-extras", action="store_true",
                    help="with --full: skip the sub-records (multi_stream, floorplans_sized, train_dp, other configs)")
    ap.add_argument("--keep-csr", action="store_true", help="re-use the CSR across steps (fwd mode)")
    ap.add_argument("--graphs", action="store_true",
                    help="fwd mode: replay a captured hipGraph per stream instead of launching every kernel "
                         "(measured: no gain at cfg 2 — with 8 streams the GPU, not the host, is the limit)")
    ap.add_argument("--precision", default="fp32", choices=["fp32", "bf16"],
                    help="storage precision.  fp32 (default) is the parity mode the headline metric is quoted in; bf16 = "
                         "the mode BASELINE.json's configs[4] names — fwd: bf16 node activations / weights with fp32 "
                         "accumulation (csrc/bf16_eval.hip); train: bf16 storage of the per-edge activations and "
                         "their gradients — use with --config 5")
    ap.add_argument("--no-side-stream", action="store_true",
                    help="train mode: every launch of the backward / forward on ONE stream (engine.SIDE_STREAM = False) — "
                         "for kernel profiles whose per-kernel times are not inflated by overlap")
    ap.add_argument("--streams", type=int, default=32,
                    help="fwd mode: independent forwards are issued round-robin on this many HIP streams "
                         "(1 = strictly one forward at a time)")
    return ap.parse_args()


def to_device(data):
    for k in ("x", "edge", "e_attr", "bbox_idx", "bbox", "labels"):
        data[k] = data[k].cuda()
    return data


DUMP_LIMIT_BYTES = 64 << 20


def dump_outputs(out_dir, arrays):
    """--dump-outputs: one DIR/<name>.npy per returned tensor, float64 kept, every other dtype as float32."""
    host = {}
    for name, t in arrays.items():
        t = t.detach()
        host[name] = (t if t.dtype == torch.float64 else t.float()).cpu().numpy()
    total = sum(a.nbytes for a in host.values())
    if total > DUMP_LIMIT_BYTES:
        raise SystemExit("--dump-outputs: %d bytes of outputs exceed the %d-byte limit" % (total, DUMP_LIMIT_BYTES))
    os.makedirs(out_dir, exist_ok=True)
    for name, a in host.items():
        np.save(os.path.join(out_dir, name + ".npy"), a)


# ---------------------------------------------------------------------------------------------
# per-op HIP-event timing (roofline of the dominant kernel)
# ---------------------------------------------------------------------------------------------
class OpTimer(object):
    """Wraps the ops.* entry points with HIP events recorded on torch's current stream — the stream
    the kernels are launched on — and accumulates per-(op, shape) time and algorithmic work."""

    def __init__(self, ops_mod):
        self.ops = ops_mod
        self.records = []
        self.orig = {}

    def _work(self, name, args, kwargs):
        o = self.ops
        if name == "linear_fwd":
            A, W = args[0], args[1]
            M, K, N = A.shape[0], A.shape[1], W.shape[0]
            return 2.0 * M * K * N, 4.0 * (M * K + N * K + M * N), "linear_fwd[%dx%d->%d]" % (M, K, N)
        if name == "edge_lin1_fwd":
            x, g, W1 = args[0], args[1], args[2]
            Cin, C, E, Nn = x.shape[1], W1.shape[0], g.E, x.shape[0]
            K = 2 * Cin + 4
            # algorithmic bytes (SURVEY.md §8 d B_agg): gathered features + indices + output
            return 2.0 * E * K * C, E * (K * 4.0 + 8) + E * C * 4.0, "edge_lin1_fwd[E=%d,K=%d]" % (E, K)
        if name == "csr_mean_fwd":
            H, g, out = args[0], args[1], args[2]
            C = out.shape[1]
            return 1.0 * g.E * C, 4.0 * (g.E * C + 2 * g.N * C) + 4.0 * g.N, "csr_mean_fwd[E=%d]" % g.E
        if name in ("segment_max_fwd", "segment_mean_fwd"):
            X, g = args[0], args[1]
            D = X.shape[1]
            return 1.0 * g.N * D, 4.0 * (g.N * D + g.P * D), "%s[D=%d]" % (name, D)
        if name == "build_graph":
            edge = args[0]
            E = max(edge.shape)
            return 0.0, 16.0 * E + 16.0 * E + 12.0 * E, "build_graph[E=%d]" % E
        if name == "linear_bwd_w":
            dY, A = args[0], args[1]
            M, Nn, K = dY.shape[0], dY.shape[1], A.shape[1]
            return 2.0 * M * K * Nn, 4.0 * (M * K + M * Nn + Nn * K), "linear_bwd_w[%dx%d^T x %d]" % (M, Nn, K)
        if name == "linear_fwd_wt":
            A, Wt = args[0], args[1]
            M, K, Nn = A.shape[0], A.shape[1], Wt.shape[1]
            return 2.0 * M * K * Nn, 4.0 * (M * K + Nn * K + M * Nn), "linear_fwd_wt[%dx%d->%d]" % (M, K, Nn)
        if name == "fusion_pool_train_fwd":
            A, lin, g = args[0], args[1], args[3]
            Nn, K, F = A.shape[0], A.shape[1], lin.weight.shape[0]
            # GEMM with the extreme-of-z epilogue + the centered K x K Gram matrix (BatchNorm statistics)
            return 2.0 * Nn * K * F + 2.0 * Nn * K * K, 4.0 * (2.0 * Nn * K + K * F + 3.0 * g.P * F), \
                "fusion_pool_train_fwd[%dx%d->%d -> P=%d]" % (Nn, K, F, g.P)
        if name == "fusion_pool_train_bwd":
            g, gZ = args[1], args[2]
            F = gZ.shape[1]
            K = 128
            # two sparse P*F-term passes (dW, dA) of K each + the K x K / F x K dense algebra + the N-row dA GEMM
            return 4.0 * g.P * F * K + 2.0 * g.N * K * K, 4.0 * (3.0 * g.P * F + 2.0 * g.N * K + 2.0 * K * F), \
                "fusion_pool_train_bwd[P=%d x %d, N=%d]" % (g.P, F, g.N)
        if name == "bn_apply_edge_sums":
            dA1, g = args[0], args[8]
            E, C = dA1.shape
            es = dA1.element_size()
            # reads dA1 and H1, writes dH1 (3 passes over [E, C]) + the attr quads + the [N, C] per-node sums
            return 22.0 * E * C, 3.0 * E * C * es + 16.0 * E + 4.0 * g.N * C, "bn_apply_edge_sums[E=%d,%dB]" % (E, es)
        return 0.0, 0.0, name

    def __enter__(self):
        for name in ("linear_fwd", "edge_lin1_fwd", "csr_mean_fwd", "segment_max_fwd", "segment_mean_fwd",
                     "build_graph", "scale_shift_relu", "bn_eval_coeffs", "linear_bwd_w", "linear_fwd_wt",
                     "fusion_pool_train_fwd", "fusion_pool_train_bwd", "bn_apply_edge_sums"):
            if not hasattr(self.ops, name):
                continue
            fn = getattr(self.ops, name)
            self.orig[name] = fn

            def wrapped(*a, _fn=fn, _name=name, **k):
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s.record()
                r = _fn(*a, **k)
                e.record()
                fl, by, label = self._work(_name, a, k)
                self.records.append((label, s, e, fl, by))
                return r
            setattr(self.ops, name, wrapped)
        # the one-kernel backward of the second edge Linear is a method (ops.BnCsrGrad.bwd_w_and_x -> yolat_bn_csr_l2_bwd):
        # dA = dY.W and dW += dY^T.A1 (2 x 2 E C^2 flops); reads Y and A, writes dA (3 passes over [E, C]) + the d_out rows
        cls = getattr(self.ops, "BnCsrGrad", None)
        if cls is not None and hasattr(cls, "bwd_w_and_x"):
            fn = cls.bwd_w_and_x
            self.orig_method = (cls, fn)

            def wrapped_m(obj, A, *a, _fn=fn, **k):
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s.record()
                r = _fn(obj, A, *a, **k)
                e.record()
                E, C = A.shape
                es = A.element_size()
                self.records.append(("bn_csr_l2_bwd%s[E=%d,%dB]" % ("_bf16" if es == 2 else "", E, es), s, e, 4.0 * E * C * C,
                                     3.0 * E * C * es + 4.0 * obj._keep[1].N * C))
                return r
            cls.bwd_w_and_x = wrapped_m
        return self

    def __exit__(self, *exc):
        for name, fn in self.orig.items():
            setattr(self.ops, name, fn)
        if getattr(self, "orig_method", None):
            cls, fn = self.orig_method
            cls.bwd_w_and_x = fn
            self.orig_method = None

    def summary(self):
        torch.cuda.synchronize()
        # per op: the MEDIAN call (and the maximum beside it).  A stall inside the timed window — an allocator growth, a
        # host hiccup between the two event records — lands in ONE call of one op; averaged as a mean it made the driver's
        # round-5 line name the wrong dominant op (fusion_pool_train_fwd at 3.5 ms per call for a 0.29 ms kernel).
        agg = {}
        for label, s, e, fl, by in self.records:
            agg.setdefault(label, ([], fl, by))[0].append(s.elapsed_time(e))
        out = {}
        for k, (ts, fl, by) in agg.items():
            ts.sort()
            n = len(ts)
            med = ts[n // 2] if n % 2 else 0.5 * (ts[n // 2 - 1] + ts[n // 2])
            out[k] = {"ms_total": med * n, "calls": n, "ms_avg": med, "ms_max": ts[-1], "ms_mean": sum(ts) / n,
                      "flops": fl, "bytes": by}
        return out


def pick_path(d, *path):
    for k in path:
        if not isinstance(d, dict) or k not in d or d[k] is None:
            return None
        d = d[k]
    return d


def plan_profile(step, n):
    """Per-stage HIP-event times of the C-side eval plan (yolat_profile_*): the events are recorded on
    the launch stream around every stage of yolat_forward_eval while `step` runs n times."""
    import ctypes
    from yolat_vectorgraphicsrecognition_amd._lib import lib
    lib.yolat_profile_reset()
    lib.yolat_profile_enable(1)
    for _ in range(n):
        step()
    torch.cuda.synchronize()
    lib.yolat_profile_enable(0)
    out = {}
    name = ctypes.create_string_buffer(128)
    ms, calls = ctypes.c_float(), ctypes.c_int()
    fl, by = ctypes.c_double(), ctypes.c_double()
    for i in range(lib.yolat_profile_count()):
        lib.yolat_profile_get(i, name, 128, ctypes.byref(ms), ctypes.byref(calls), ctypes.byref(fl), ctypes.byref(by))
        out[name.value.decode()] = {"ms_total": ms.value, "calls": calls.value, "ms_avg": ms.value / max(calls.value, 1),
                                    "flops": fl.value, "bytes": by.value}
    lib.yolat_profile_reset()
    return out


# HBM/fabric bytes per launch of the roofline kernel: read from profiles/pmc_traffic.json, which tools/pmc_traffic.sh
# regenerates on the GPU box from separate rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of this same command
# (FETCH_SIZE doubled per the gfx950 note in MI355X_MICROARCH.md section HBM).  Every entry records the sha256 of the
# kernel sources it was measured on; when the sources have changed since, the entry is STALE and `traffic` is null.
def _source_digest(files):
    import hashlib
    h = hashlib.sha256()
    for f in files:
        with open(os.path.join(REPO, f), "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()[:16]


def pmc_traffic(stage_label, cfg):
    path = os.path.join(REPO, "profiles", "pmc_traffic.json")
    if not os.path.exists(path):
        return None, "no profiles/pmc_traffic.json"
    try:
        table = json.load(open(path))
    except ValueError:
        return None, "profiles/pmc_traffic.json unreadable"
    ent = table.get("cfg%s" % cfg, {}).get(stage_label)
    if ent is None:
        return None, "no PMC pass recorded for this stage at cfg %s" % cfg
    if ent.get("source_digest") != _source_digest(ent.get("sources", [])):
        return None, "STALE: %s changed since %s was measured" % (", ".join(ent.get("sources", [])), ent.get("file"))
    return 2.0 * ent["fetch_kib"] * 1024 + ent["write_kib"] * 1024, ent.get("file")


def roofline_entry(summary, cfg=None, precision="fp32", shape=None):
    r = _roofline_entry(summary)
    if cfg is not None:
        r["traffic"], r["traffic_source"] = pmc_traffic(r["kernel"], cfg)
        r["algorithmic_bytes"] = summary[r["kernel"]]["bytes"]
    r.update(executed_pricing(r["kernel"], summary[r["kernel"]], precision, shape))
    return r


def utilisation_view(r):
    """Sub-record form of a roofline entry: `frac` is a UTILISATION figure that cannot exceed what
    the hardware did, everything priced on work the kernel never moved or issued is named `credit_*`.
      bound hbm : frac = counter traffic / t / 8 TB/s when a PMC pass exists for the stage (`hbm_frac_counters`), else the
                  bytes the kernel has to move (`executed_bytes`) / t / 8 TB/s; `credit_b_agg_of_hbm_peak` = SURVEY 8(d)'s
                  algorithmic bytes of the unfactorised reference op / t / 8 TB/s (the figure north_star's ">= 50 % HBM
                  roofline on the sparse aggregation" is quoted on; it credits the factorisation and the fusion).
      bound mfma: frac = flops ISSUED on the pipe they are issued to / that pipe's dense peak (`frac_executed_pipe`);
                  `credit_algorithmic_of_fp32_peak` = algorithmic fp32 flops / t / fp32-MFMA peak (may exceed 1 for a
                  GEMM emulated with six bf16 products)."""
    r = dict(r)
    t = r["avg_launch_us"] * 1e-6
    alg = r.pop("frac")
    r.pop("frac_algorithmic", None)
    r["hbm_frac_counters"] = (r["traffic"] / t / (PEAK_HBM_GBS * 1e9)) if r.get("traffic") else None
    if r["bound"] == "hbm":
        r["credit_b_agg_of_hbm_peak"] = alg
        must = r.get("executed_bytes", r.get("algorithmic_bytes", 0.0)) / t / (PEAK_HBM_GBS * 1e9)
        r["frac"] = r["hbm_frac_counters"] if r["hbm_frac_counters"] is not None else min(must, alg)
        r["frac_kind"] = ("HBM bytes by PMC counters / t / 8 TB/s" if r["hbm_frac_counters"] is not None else
                          "bytes the kernel must move / t / 8 TB/s (no PMC pass for this stage)")
    else:
        r["credit_algorithmic_of_fp32_peak"] = alg
        r["frac"] = r["frac_executed_pipe"]
        r["frac_kind"] = "flops issued / dense peak of the pipe they are issued to (%s)" % r.get("executed_pipe", "")
    r["achieved_note"] = "`achieved` is algorithmic work / t (credit); `frac` is the utilisation figure"
    return r


def _runs_as_bf16x6(label, precision, shape):
    """Which stages of the fp32 eval plan execute their GEMM as six exact-split bf16 MFMA products (x6.hpp)."""
    if precision != "fp32" or shape is None:
        return False
    N, E, P = shape
    if label.startswith("fusion_gemm+segmax"):
        return os.environ.get("YOLAT_STRICT_FP32", "0") != "1"
    if label.startswith("edge_uv_mlp2_mean"):
        return E >= 131072
    if label.startswith("cls1"):
        return P >= 1024 and os.environ.get("YOLAT_STRICT_FP32", "0") != "1"
    if label.startswith("node_uv"):
        return N >= 65536
    return False


def executed_pricing(label, rec, precision, shape):
    """Both roofline fractions of one stage, side by side at the top level of the entry:
      frac_algorithmic   — SURVEY 8(d): max(algorithmic bytes / HBM peak, algorithmic flops / MFMA peak of the dtype the
                           reference computes in) / t.  For an fp32 GEMM that is the fp32-input MFMA peak, 157.3 TFLOP/s.
      frac_executed_pipe — the same with the flops the kernel really ISSUES priced on the pipe it issues them to: an
                           fp32 GEMM emulated with six exact-split bf16 products is 6x the flops on the 2.5 PFLOP/s dense
                           bf16 pipe.  This is the utilisation figure; frac_algorithmic above it is credit for the
                           emulation (it may exceed the executed figure by 157.3*6/2500 = 2.65x)."""
    t = rec["ms_avg"] * 1e-3
    fl, by = rec["flops"], rec["bytes"]
    alg_peak = PEAK_MFMA_BF16_TFLOPS if precision == "bf16" and "bf16" in label else PEAK_MFMA_F32_TFLOPS
    frac_alg = max(by / (PEAK_HBM_GBS * 1e9), fl / (alg_peak * 1e12)) / t
    ex_by = by
    if label.startswith("edge_uv_mlp2_mean") and shape is not None:
        # the fused, factorised edge kernel: the stage's byte count is B_agg of the unfactorised layer (credit for the
        # algebra); what it must move is the per-node products once, attr + indices per edge, and the output rows
        N, E, P = shape
        s = 2.0 if "bf16" in label else 4.0
        ex_by = N * 128 * s + E * 24.0 + (2.0 if s == 4.0 else 1.5) * N * 64 * 4.0 + 4.0 * N
    t_b = ex_by / (PEAK_HBM_GBS * 1e9)
    x6 = _runs_as_bf16x6(label, precision, shape)
    if label.startswith("conv_local") and shape is not None:
        # the one-launch conv stack (csrc/conv_local.hip) issues 24 v_mfma_f32_32x32x16_bf16 per 32 edges and layer (8 of
        # them identity products that transpose / add the gathered rows, 2 the attr term, 2 the shift, 8 the second Linear,
        # 4 the mean aggregation) = 24 576 flops per edge against 2 (4 C + C C) = 8 704 algorithmic ones, and the node side
        # as issued; the stage's byte count is already what it has to move (x, ids, e_attr in; feats + pooled rows out)
        N, E, P = shape
        ex_fl = fl * (24576.0 * E + 32768.0 * N) / (8704.0 * E + 32768.0 * N)
        ex_peak, pipe = PEAK_MFMA_BF16_TFLOPS, "bf16 MFMA (24 per 32 edges and layer, 8.7 of 24.6 kflop per edge algorithmic)"
    elif x6:
        ex_fl, ex_peak, pipe = 6.0 * fl, PEAK_MFMA_BF16_TFLOPS, "bf16 MFMA (fp32 GEMM as six exact-split bf16 products)"
    elif alg_peak == PEAK_MFMA_BF16_TFLOPS:
        ex_fl, ex_peak, pipe = fl, PEAK_MFMA_BF16_TFLOPS, "bf16 MFMA"
    else:
        ex_fl, ex_peak, pipe = fl, PEAK_MFMA_F32_TFLOPS, "fp32 MFMA"
    frac_ex = max(t_b, ex_fl / (ex_peak * 1e12)) / t
    return {"frac_algorithmic": frac_alg, "frac_executed_pipe": frac_ex, "executed_pipe": pipe,
            "executed_flops": ex_fl, "algorithmic_flops": fl, "executed_bytes": ex_by}


PEAK_MFMA_BF16_TFLOPS = 2500.0   # dense bf16 MFMA peak (MI355X_MICROARCH.md; AMD's 5 PF figure is 2:1 sparse)


def _roofline_entry(summary):
    label, rec = max(summary.items(), key=lambda kv: kv[1]["ms_total"])
    t = rec["ms_avg"] * 1e-3
    intensity = rec["flops"] / max(rec["bytes"], 1.0)
    peak = PEAK_MFMA_BF16_TFLOPS if "bf16" in label else PEAK_MFMA_F32_TFLOPS
    ridge = peak * 1e12 / (PEAK_HBM_GBS * 1e9)
    if intensity >= ridge:
        ach = rec["flops"] / t / 1e12
        return {"kernel": label, "bound": "mfma", "achieved": ach, "peak": peak,
                "unit": "TFLOP/s", "frac": ach / peak, "traffic": None,
                "avg_launch_us": rec["ms_avg"] * 1e3}
    ach = rec["bytes"] / t / 1e9
    return {"kernel": label, "bound": "hbm", "achieved": ach, "peak": PEAK_HBM_GBS, "unit": "GB/s",
            "frac": ach / PEAK_HBM_GBS, "traffic": None, "avg_launch_us": rec["ms_avg"] * 1e3}


PEAK_MFMA_BF16_RANDOM_TFLOPS = 1870.0   # measured: v_mfma_f32_32x32x16_bf16 every 17.5 ns per SIMD on full-entropy
                                        # operands, all 256 CUs busy (tools/exp/mfma_rate.hip; 13.6 ns on constants)


def fusion_stage_roofline(summary, cfg, precision):
    """The fusion stage of the eval plan (fusion_block + per-proposal max | fusion_block_super, one launch): the stage
    that led the cfg-2 profile until round 2.  `frac` prices the ALGORITHMIC fp32 flops (2 (N+P) D F) against the
    fp32-input MFMA peak, as SURVEY 8(d) prescribes for the reference's op; on the default fp32 path the kernel executes
    them as six bf16 MFMA products per k (`executed`: 6x the flops against the dense bf16 peak and against the measured
    random-operand issue rate)."""
    label = next((k for k in summary if k.startswith("fusion_gemm+segmax")), None)
    if label is None:
        return None
    rec = summary[label]
    t = rec["ms_avg"] * 1e-3
    ach = rec["flops"] / t / 1e12
    out = {"kernel": label, "bound": "mfma", "achieved": ach, "peak": PEAK_MFMA_F32_TFLOPS, "unit": "TFLOP/s",
           "frac": ach / PEAK_MFMA_F32_TFLOPS, "avg_launch_us": rec["ms_avg"] * 1e3,
           "algorithmic_flops": rec["flops"], "algorithmic_bytes": rec["bytes"]}
    out["traffic"], out["traffic_source"] = pmc_traffic(label, cfg)
    if precision == "fp32" and os.environ.get("YOLAT_STRICT_FP32", "0") != "1":
        x = 6.0 * rec["flops"]
        out["executed"] = {"bf16_mfma_flops": x, "bf16_TFLOPs": x / t / 1e12,
                           "frac_of_dense_bf16_peak": x / t / 1e12 / PEAK_MFMA_BF16_TFLOPS,
                           "frac_of_measured_random_operand_rate": x / t / 1e12 / PEAK_MFMA_BF16_RANDOM_TFLOPS,
                           "note": "fp32 GEMM emulated with six exact-split bf16 products per k, fp32 accumulate "
                                   "(fusion_x6.hip); frac above 1 against the fp32-MFMA peak would be credit for the "
                                   "emulation, not pipe utilisation"}
    return out


def aggregation_roofline(cfg_name="5", C=64, reps=20):
    """HBM roofline of the sparse aggregation kernel (csr_mean: per-node mean over the CSR edge range,
    torch_vertex.py:333-335 'mean' aggr) on a cfg-5-sized graph, where the E x C message matrix (307 MB)
    does not fit in L2/MALL.  Algorithmic bytes per launch = E*C*4 (messages) + N*C*4 (output) +
    (N+1)*4 (row_ptr); timed with HIP events on the launch stream."""
    import yolat_vectorgraphicsrecognition_amd as yv
    data, _, _, _ = yv.config(cfg_name)
    g = yv.ops.build_graph(data.edge.cuda(), data.e_attr.cuda(), data.bbox_idx.cuda(), int(data.x.shape[0]),
                           int(data.bbox.shape[0]))
    E, N = g.E, g.N
    H = torch.randn(E, C, device="cuda")
    sc, sh = torch.rand(C, device="cuda") + 0.5, torch.randn(C, device="cuda")
    out = torch.empty(N, C, device="cuda")
    for _ in range(3):
        yv.ops.csr_mean_fwd(H, g, out, h_pro=(sc, sh), h_relu=True)
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        yv.ops.csr_mean_fwd(H, g, out, h_pro=(sc, sh), h_relu=True)
    e.record()
    torch.cuda.synchronize()
    t = s.elapsed_time(e) * 1e-3 / reps
    by = 4.0 * (E * C + N * C + N + 1)
    ach = by / t / 1e9
    return {"kernel": "csr_mean_fwd[E=%d x C=%d -> N=%d] (BN+ReLU prologue fused)" % (E, C, N), "bound": "hbm",
            "achieved": ach, "peak": PEAK_HBM_GBS, "unit": "GB/s", "frac": ach / PEAK_HBM_GBS, "traffic": None,
            "avg_launch_us": t * 1e6, "bytes_per_launch": by}


def edge_layer_roofline(cfg_name="5", reps=10):
    """Roofline of the fused, factorised edge kernel of a block layer (gather-add of the per-node products + BN/ReLU
    + second Linear + BN/ReLU + mean aggregation: everything `propagate(aggr='mean')` does, torch_vertex.py:324) on
    a cfg-5-sized graph.  Reported as SURVEY.md section 8(d) prescribes for a fused kernel: max(bytes/BW, flops/peak)/t with
    the ALGORITHMIC aggregation bytes of the unfactorised layer, B_agg = E*((2*Cin+4)*4 + 8) + N*C*4, and its edge-MLP
    flops F_edge = 2*E*((2*Cin+4)*C + C*C)."""
    import ctypes
    import yolat_vectorgraphicsrecognition_amd as yv
    from yolat_vectorgraphicsrecognition_amd._lib import lib, check
    data, _, _, _ = yv.config(cfg_name)
    g = yv.ops.build_graph(data.edge.cuda(), data.e_attr.cuda(), data.bbox_idx.cuda(), int(data.x.shape[0]),
                           int(data.bbox.shape[0]))
    E, N, C, Cin = g.E, g.N, 64, 64
    gen = torch.Generator().manual_seed(0)
    UV = torch.randn(N, 2 * C, generator=gen).cuda()
    W2 = (torch.randn(C, C, generator=gen) / 8).cuda()
    wc4 = torch.randn(C, 4, generator=gen).cuda()
    vec = [torch.randn(C, generator=gen).cuda() for _ in range(6)]
    f_out = torch.zeros(N, C, device="cuda")
    st = torch.cuda.current_stream().cuda_stream

    def run():
        check(lib.yolat_edge_uv_mlp2_mean_eval(UV.data_ptr(), 2 * C, g.src.data_ptr(), g.dst.data_ptr(), g.attr.data_ptr(),
                                               g.row_ptr.data_ptr(), N, E, wc4.data_ptr(), vec[0].data_ptr(),
                                               vec[1].data_ptr(), vec[2].data_ptr(), W2.data_ptr(), vec[3].data_ptr(),
                                               vec[4].data_ptr(), vec[5].data_ptr(), C, f_out.data_ptr(), C, st))
    for _ in range(3):
        run()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        run()
    e.record()
    torch.cuda.synchronize()
    t = s.elapsed_time(e) * 1e-3 / reps
    b_agg = E * ((2 * Cin + 4) * 4.0 + 8) + N * C * 4.0
    f_edge = 2.0 * E * ((2 * Cin + 4) * C + C * C)
    t_bytes, t_flops = b_agg / (PEAK_HBM_GBS * 1e9), f_edge / (PEAK_MFMA_F32_TFLOPS * 1e12)
    # what the kernel really executes (factorised first Linear; at this size layer 2 runs as an fp32 GEMM emulated with
    # six bf16 MFMA products): compulsory HBM bytes = UV once + attr + indices + f_out read-modify-write
    x_bytes = N * 2 * C * 4.0 + E * (16.0 + 8.0) + 2.0 * N * C * 4.0 + 4.0 * N
    x_flops_f32 = 2.0 * E * (4 * C + C * C)
    x_flops_bf16 = 6.0 * 2.0 * E * C * C
    x_bound = max(x_bytes / (PEAK_HBM_GBS * 1e9), x_flops_bf16 / (PEAK_MFMA_BF16_TFLOPS * 1e12))
    out = {"kernel": "edge_uv_mlp2_mean[E=%d, N=%d, C=%d] (factorised edge MLP + mean aggregation, one kernel)" % (E, N, C),
           "traffic": None, "avg_launch_us": t * 1e6, "algorithmic_bytes": b_agg, "algorithmic_flops": f_edge,
           "hbm_equivalent_GBs": b_agg / t / 1e9, "frac": max(t_bytes, t_flops) / t,
           "note": "credit_algorithmic_frac / achieved: SURVEY 8(d) pricing of a fused kernel, max(bytes/BW, flops/peak)/t with "
                   "the bytes / flops of the UNFACTORISED layer (B_agg, F_edge) — credit for the algebra, not pipe "
                   "utilisation; `executed` prices the work the kernel really does",
           "executed": {"compulsory_bytes": x_bytes, "hbm_GBs": x_bytes / t / 1e9,
                        "hbm_frac": x_bytes / t / 1e9 / PEAK_HBM_GBS,
                        "fp32_equivalent_flops": x_flops_f32, "fp32_equivalent_TFLOPs": x_flops_f32 / t / 1e12,
                        "bf16_mfma_flops": x_flops_bf16, "bf16_mfma_frac": x_flops_bf16 / t / 1e12 / PEAK_MFMA_BF16_TFLOPS,
                        "frac_of_executed_bound": x_bound / t,
                        "limiter": "VALU issue (PMC: profiles/r04_fwd_cfg5_pmc_sq_a.txt, _b.txt: SQ_ACTIVE_INST_VALU 56 % of "
                                   "SQ_BUSY_CYCLES x 8; operand splits + gather-add + epilogue), not HBM or the matrix cores"}}
    if t_flops > t_bytes:
        out.update(bound="mfma", achieved=f_edge / t / 1e12, peak=PEAK_MFMA_F32_TFLOPS, unit="TFLOP/s")
    else:
        out.update(bound="hbm", achieved=b_agg / t / 1e9, peak=PEAK_HBM_GBS, unit="GB/s")
    # like the sub-records (utilisation_view): `frac` is a utilisation figure (<= 1), what is priced on the unfactorised
    # layer's algorithmic work is credit
    out["credit_algorithmic_frac"] = out.pop("frac")
    out["frac"] = out["executed"]["frac_of_executed_bound"]
    out["frac_kind"] = "max(compulsory bytes / 8 TB/s, bf16 MFMA flops issued / 2.5 PF) / t: the executed work against its bound"
    out["achieved_note"] = "`achieved` is algorithmic work / t (credit); `frac` is the utilisation figure"
    return out


# ---------------------------------------------------------------------------------------------
# CPU baseline: the op-for-op torch oracle on the host cores (bounded sample)
# ---------------------------------------------------------------------------------------------
def cpu_baseline(cfg_name, optkw, mode, budget_s=25, thread_counts=(8, 16, 32, 64)):
    from oracle import oracle_torch as orc
    import yolat_vectorgraphicsrecognition_amd as yv
    sys.path.insert(0, os.path.join(REPO, "tests"))
    import golden_util as gu
    data, slices, _, n_graphs = yv.config(cfg_name)
    opt = orc.Opt(**optkw)
    model = gu.fill_state_(orc.SparseCADGCN(opt), 0)
    crit = orc.DetectionLoss(opt)
    ncpu = os.cpu_count() or 1
    best = None
    budget_t0 = time.time()
    for threads in [t for t in thread_counts if t <= ncpu] or [ncpu]:
        torch.set_num_threads(threads)
        if mode == "fwd":
            model.eval()

            def run():
                with torch.no_grad():
                    model(data, None)
        else:
            model.train()
            optim = torch.optim.Adam(model.parameters(), lr=2.5e-4, weight_decay=1e-5)

            def run():
                orc.train_step(model, crit, optim, data)
        reps = 10 if mode == "fwd" else 3
        for _ in range(2):
            run()
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            run()
            ts.append(time.perf_counter() - t0)
        ts.sort()
        med = ts[len(ts) // 2]
        if best is None or med < best[0]:
            best = (med, threads, reps)
        if time.time() - budget_t0 > budget_s:
            break
    med, threads, reps = best
    return {"value": n_graphs / med, "unit": "graphs/s", "cores": threads, "kind": "port",
            "ms_per_step": med * 1e3, "host_cpus": ncpu,
            "sample": "cfg %s, %s, median of %d steps of the op-for-op torch oracle (fp32), best of "
                      "thread counts {%s}<=cpu_count" % (cfg_name, mode, reps, ",".join(str(t) for t in thread_counts))}


# ---------------------------------------------------------------------------------------------
# sub-records of the N = 1 line / the N > 1 line
# ---------------------------------------------------------------------------------------------
def multi_stream_throughput(model, data, slices, n_graphs, n_streams=32, forwards=1024, keep_csr=False):
    """graphs/s with `n_streams` independent forwards in flight (round-robin over HIP streams), measured over
    `forwards` (>= 512) complete forwards regardless of --steps: the serving-style throughput of one GPU."""
    streams = [torch.cuda.Stream() for _ in range(n_streams)]

    def one(i):
        if not keep_csr:
            data._yolat_stage = None
        with torch.cuda.stream(streams[i % n_streams]), torch.no_grad():
            model(data, slices)

    for i in range(3 * n_streams):          # per-stream plans: fold / split weights, workspaces
        one(i)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(forwards):
        one(i)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    return {"value": n_graphs * forwards / dt, "unit": "graphs/s", "streams": n_streams, "forwards": forwards,
            "us_per_forward": dt / forwards * 1e6}


def floorplans_sized_record(yv, gu, cpu=True):
    """cfg 1 (BASELINE.json configs[0]: one Floorplans-sized graph, P = 2000 proposals, N ~ 44k, E ~ 53k) on this GPU
    next to the CPU oracle on the same graph — north_star's ">= 10x the CPU-reference graphs/s on Floorplans-sized
    graphs at 1 GPU" as a measured pair."""
    data, slices, optkw, n_graphs = yv.config("1")
    N, E, P = data.x.shape[0], data.edge.shape[0], data.bbox.shape[0]
    model = gu.fill_state_(yv.SparseCADGCN(yv.Opt(**optkw)), 0).cuda().eval()
    to_device(data)

    def one():
        data._yolat_stage = None
        with torch.no_grad():
            return model(data, slices)[0]

    for _ in range(5):
        one()
    torch.cuda.synchronize()
    n = 100
    t0 = time.perf_counter()
    for _ in range(n):
        one()
    torch.cuda.synchronize()
    lat = (time.perf_counter() - t0) / n
    ms = multi_stream_throughput(model, data, slices, n_graphs, n_streams=16, forwards=512)
    rec = {"workload": "cfg1 eval forward: Floorplans-sized synthetic Bezier graph", "nodes": N, "edges": E,
           "proposals": P, "ms_per_forward": lat * 1e3, "graphs_per_sec_one_at_a_time": n_graphs / lat,
           "graphs_per_sec_16_streams": ms["value"]}
    if cpu:
        c = cpu_baseline("1", optkw, "fwd", budget_s=12)
        rec["cpu_baseline"] = c
        rec["speedup_vs_cpu_one_at_a_time"] = rec["graphs_per_sec_one_at_a_time"] / c["value"]
        rec["speedup_vs_cpu_16_streams"] = rec["graphs_per_sec_16_streams"] / c["value"]
    return rec


def _timed_loop(fn, budget_s, lo=5, hi=200, warm=5):
    """Run `fn` warm times, then as many times as fit in about budget_s seconds (lo..hi); seconds per call."""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    one = max(time.perf_counter() - t0, 1e-5)
    n = int(max(lo, min(hi, budget_s / one)))
    # four timed chunks, the median chunk's mean: one allocator growth or host hiccup inside the region does not end up
    # in the figure (a whole slow region still does)
    chunk = max(1, n // 4)
    means = []
    for _ in range(4):
        t0 = time.perf_counter()
        for _ in range(chunk):
            fn()
        torch.cuda.synchronize()
        means.append((time.perf_counter() - t0) / chunk)
    means.sort()
    return 0.5 * (means[1] + means[2]), 4 * chunk


def eval_config_record(yv, gu, cfg, precision, budget_s=4.0):
    """One more BASELINE.json configuration inside the N = 1 line: eval forward of `cfg` in `precision`, one forward at
    a time (CSR rebuilt every forward), its stage table and the dominant stage priced both ways."""
    data, slices, optkw, n_graphs = yv.config(cfg)
    N, E, P = int(data.x.shape[0]), int(data.edge.shape[0]), int(data.bbox.shape[0])
    model = gu.fill_state_(yv.SparseCADGCN(yv.Opt(**optkw)), 0).cuda().eval()
    model.set_eval_precision(precision)
    to_device(data)

    def one():
        data._yolat_stage = None
        with torch.no_grad():
            return model(data, slices)[0]

    lat, n = _timed_loop(one, budget_s)
    table = plan_profile(one, 20)
    roof = utilisation_view(roofline_entry(table, str(cfg), precision, (N, E, P)))
    stages = {k: round(v["ms_avg"] * 1e3, 1) for k, v in sorted(table.items(), key=lambda kv: -kv[1]["ms_total"])}
    priced = {}
    for k, v in table.items():
        if v["ms_avg"] * 1e3 >= 20.0:
            e = executed_pricing(k, v, precision, (N, E, P))
            priced[k] = {"us": round(v["ms_avg"] * 1e3, 1), "frac": round(e["frac_executed_pipe"], 3),
                         "credit_algorithmic": round(e["frac_algorithmic"], 3), "executed_pipe": e["executed_pipe"]}
    total_fl = sum(v["flops"] * v["calls"] for v in table.values()) / 20.0
    del model
    return {"workload": "cfg%s eval forward, %s" % (cfg, "fp32" if precision == "fp32" else
                                                   "bf16 storage / fp32 accumulate"),
            "nodes": N, "edges": E, "proposals": P, "n_blocks": optkw["n_blocks"], "forwards_timed": n,
            "ms_per_forward": lat * 1e3, "graphs_per_sec": n_graphs / lat,
            "algorithmic_GFLOP_per_forward": total_fl / 1e9, "end_to_end_TFLOPs": total_fl / lat / 1e12,
            "gpu_us_sum_of_stages": round(sum(v["ms_total"] for v in table.values()) / 20.0 * 1e3, 1),
            "roofline": roof, "stages_us": stages, "stages_priced": priced}


def train_config_record(yv, gu, cfg, precision="fp32", budget_s=5.0, cpu=True):
    """BASELINE.json configs[2] (cfg 3) — or any training configuration — inside the N = 1 line: Trainer.step
    (forward + CE + backward + Adam, CSR rebuilt every step) with its own CPU baseline and dominant-op roofline."""
    data, slices, optkw, n_graphs = yv.config(cfg)
    N, E, P = int(data.x.shape[0]), int(data.edge.shape[0]), int(data.bbox.shape[0])
    opt = yv.Opt(**optkw)
    model = gu.fill_state_(yv.SparseCADGCN(opt), 0).cuda()
    to_device(data)
    trainer = yv.Trainer(model, opt, lr=2.5e-4, weight_decay=1e-5, precision=precision)

    def step():
        data._yolat_stage = None
        return trainer.step(data, slices)

    t, n = _timed_loop(step, budget_s, lo=5, hi=100, warm=4)
    from yolat_vectorgraphicsrecognition_amd import engine as _eng
    from yolat_vectorgraphicsrecognition_amd import trainer as _trn
    plan_steps = trainer.plan_steps
    # host side of a step: the time trainer.step() takes to RETURN (enqueue only; the GPU is drained outside the timed
    # region), through the one-call plan (yolat_train_step) and through the Python schedule it replaces
    def host_ms(flag):
        old = _trn.TRAIN_PLAN
        _trn.TRAIN_PLAN = flag
        try:
            step()
            torch.cuda.synchronize()
            ts = []
            for _ in range(9):
                t0 = time.perf_counter()
                step()
                ts.append(time.perf_counter() - t0)
                torch.cuda.synchronize()
        finally:
            _trn.TRAIN_PLAN = old
        ts.sort()
        return ts[len(ts) // 2] * 1e3
    host_plan, host_python = host_ms(True), host_ms(False)
    side_probe = dict(_eng.SIDE_PROBE.get(torch.cuda.current_device(), {})) or None
    # per-op times with every launch on ONE stream: with the weight gradients and node branches on the second stream
    # (the default, which `ms_per_step` above is measured with) the HIP events around an op also cover whatever the other
    # stream runs beside it, and per-op times stop meaning anything (profiles/r04_train_cfg3_kernel_stats.txt)
    side = yv.engine.SIDE_STREAM
    yv.engine.SIDE_STREAM = False
    _trn.TRAIN_PLAN = False              # the op table times the ops.* entry points: the Python schedule issues them
    try:
        for _ in range(2):
            step()
        with OpTimer(yv.ops) as timer:
            for _ in range(10):
                step()
            table = timer.summary()
    finally:
        yv.engine.SIDE_STREAM = side
        _trn.TRAIN_PLAN = True
    roof = roofline_entry(table, None, precision)
    roof["note"] = ("dominant op of the step by HIP-event time, all launches on one stream (ops.* entry points; each is one "
                    "or a few launches)")
    nb, C, D, F = optkw["n_blocks"], 64, 128, 1024
    K = optkw["n_classes"]
    fwd = (2.0 * E * (14 * C + C * C) + 2.0 * E * ((2 * C + 4) * C + C * C) * (nb - 1) + 4.0 * N * 5 * C
           + 4.0 * N * C * C * (nb - 1) + 2.0 * (N + P) * D * F + 2.0 * P * (2304 * 512 + 512 * 256 + 256 * K))
    top = sorted(table.items(), key=lambda kv: -kv[1]["ms_total"])[:6]
    rec = {"workload": "cfg%s train step (fwd+CE+bwd+Adam), %d graph(s) per step, %s" %
                       (cfg, n_graphs, "fp32" if precision == "fp32" else "bf16 storage of the per-edge tensors"),
           "nodes": N, "edges": E, "proposals": P, "steps_timed": n, "ms_per_step": t * 1e3, "side_stream_probe": side_probe,
           "one_call_plan": {"steps_through_yolat_train_step": plan_steps, "host_ms_per_step": round(host_plan, 4),
                             "host_ms_per_step_python_schedule": round(host_python, 4),
                             "note": "ms_per_step is measured through the plan when steps_through_yolat_train_step > 0; host "
                                     "ms = time for Trainer.step to return, GPU drained between steps"},
           "graphs_per_sec": n_graphs / t,
           "whole_step": {"algorithmic_GFLOP": 3.0 * fwd / 1e9, "TFLOPs": 3.0 * fwd / t / 1e12,
                          "frac_of_fp32_mfma_peak": 3.0 * fwd / t / 1e12 / PEAK_MFMA_F32_TFLOPS,
                          "note": "3 x the unfactorised forward flops of SURVEY 8(d) over the step time"},
           "roofline": roof,
           "op_breakdown_us": {k: round(v["ms_total"] / 10.0 * 1e3, 1) for k, v in top},
           "op_breakdown_us_per_call": {k: round(v["ms_avg"] * 1e3, 1) for k, v in top},
           "op_breakdown_us_max_call": {k: round(v["ms_max"] * 1e3, 1) for k, v in top},
           "setup_steps": {"warm": 4, "untimed_after_stream_switch": 2, "op_table_steps": 10},
           "op_breakdown_note": "per step / per call = the MEDIAN call of each op x calls per step (the slowest call beside "
                                "it), one-stream schedule (engine.SIDE_STREAM off for this table only, two untimed steps "
                                "after the switch)"}
    agg_calls = [v for k, v in table.items() if k.startswith("csr_mean_fwd")]
    if agg_calls:
        # the training aggregation kernel INSIDE the step (median call): what `roofline_aggregation` is quoted on
        rec["csr_mean_fwd_us_per_call_in_step"] = round(max(v["ms_avg"] for v in agg_calls) * 1e3, 1)
    del trainer, model
    if cpu:
        c = cpu_baseline(cfg, optkw, "train", budget_s=10, thread_counts=(32,))
        rec["cpu_baseline"] = c
        rec["speedup_vs_cpu"] = rec["graphs_per_sec"] / c["value"]
    return rec


def _reference_timings():
    """tests/golden/reference_timings.json: the reference's OWN _get_proposal / non_max_suppression timed in the build
    container by tests/golden/time_reference.py (the reference does not travel to the GPU box; its numbers do)."""
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "tests", "golden", "reference_timings.json")
    try:
        with open(path) as f:
            return json.load(f)
    except (OSError, ValueError):
        return {}


def proposals_record(yv):
    """box-proposal generation (Datasets/graph_dict3.py:309-789) on one synthetic per-SVG dict of Floorplans
    size — ms per SVG, split into the native core (yolat_proposals_build: grid windows, de-duplication, edge pick-up,
    rejection tests) and the per-proposal assembly (yolat_proposals_assemble, round 6; `ms_per_svg_python_assembly_loop` =
    the Python loop it replaced) + the proposal tree, with and without the 13 unused statistics (:644-705).  HOST code
    (DataLoader workers, cached per SVG :924-929): one thread, like the reference."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tests"))
    import proposals_util as pu
    from yolat_vectorgraphicsrecognition_amd import proposals as pr
    gd, gt_bbox, gt_labels, step, n_classes = pu.synth_graph_dict(**pu.TIMING_CASE)

    def med(fn, reps=5):
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            out = fn()
            ts.append(time.perf_counter() - t0)
        ts.sort()
        return ts[len(ts) // 2], out

    t_full, res = med(lambda: pr.get_proposal(gd, gt_bbox, gt_labels, bbox_sampling_step=step, n_classes=n_classes))
    t_nostat, _ = med(lambda: pr.get_proposal(gd, gt_bbox, gt_labels, bbox_sampling_step=step, n_classes=n_classes,
                                              stat_feats=False))
    # the native core alone, on the renumbered inputs get_proposal hands it
    is_control = np.asarray(gd["attr"]["is_control"])
    keep = (is_control == 0)[:, 0]
    o2n = np.cumsum(keep) - 1
    pos = np.asarray(gd["pos"]["spatial"])[keep]
    edge = o2n[np.asarray(gd["edge"]["shape"]).reshape(-1, 2)]
    sedge = o2n[np.asarray(gd["edge"]["super"]).reshape(-1, 2)]
    cc = [[int(o2n[i]) for i in c] for c in gd["cc"]]
    t_core, w = med(lambda: pr.proposal_windows(pos, cc, edge, sedge, step))
    t_py, _ = med(lambda: pr.get_proposal(gd, gt_bbox, gt_labels, bbox_sampling_step=step, n_classes=n_classes, native=False), 3)
    ref = _reference_timings().get("get_proposal", {})
    rec = {"workload": "one synthetic per-SVG graph dict (proposals_util.TIMING_CASE): %d proposals, %d nodes, %d edges out"
                       % (int(np.asarray(res[9]).shape[0]), int(res[0].shape[0]), int(res[3].shape[0])),
           "ms_per_svg": t_full * 1e3, "ms_per_svg_without_stat_feats": t_nostat * 1e3,
           "ms_native_core_yolat_proposals_build": t_core * 1e3, "ms_assembly_and_tree": (t_full - t_core) * 1e3,
           "ms_per_svg_python_assembly_loop": t_py * 1e3,
           "threads": 1,
           "reference_ms_per_svg_build_container": (ref.get("seconds_per_svg") or 0) * 1e3 or None,
           "reference_proposals": ref.get("proposals"),
           "note": "reference = its own _get_proposal compiled from source, timed by tests/golden/time_reference.py in the "
                   "build container (a different host than this box: a reported baseline, not a same-box ratio)"}
    if ref.get("seconds_per_svg"):
        rec["x_reference"] = ref["seconds_per_svg"] / t_full
    return rec


def nms_record(yv):
    """the reference's class-aware non_max_suppression (cad_recognition/train.py:34-121; the evaluation
    loop's call :448, conf_thres 0) on 10 000 candidates (625 boxes x 16 classes): postprocess.non_max_suppression over
    the device nms kernel (csrc/nms.hip), ms per call with the prediction resident on the GPU."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tests"))
    import proposals_util as pu
    from yolat_vectorgraphicsrecognition_amd import postprocess as pp
    cs = pu.NMS_TIMING
    rng = np.random.default_rng(cs["seed"])
    n, nc = cs["n"], cs["nc"]
    # (the generator of tests/golden/make_golden_post.synth_prediction, restated: the golden scripts do not travel as imports)
    centers = rng.random((max(n // 6, 1), 2)) * 800.0
    c = centers[rng.integers(0, len(centers), size=n)] + rng.normal(0, 6.0, size=(n, 2))
    wh = 20 + rng.random((n, 2)) * 60
    box = np.concatenate([c - wh / 2, c + wh / 2], 1)
    obj = rng.random((n, 1))
    logits = rng.normal(0, 2.0, size=(n, nc))
    cls = np.exp(logits) / np.exp(logits).sum(1, keepdims=True)
    pred = torch.from_numpy(np.concatenate([box, obj, cls], 1).astype(np.float32)[None]).cuda()

    def one():
        return pp.non_max_suppression(pred, conf_thres=0.0, iou_thres=0.5)

    t, _ = _timed_loop(one, 2.0, lo=5, hi=200, warm=3)
    det = one()
    ref = _reference_timings().get("non_max_suppression", {})
    rec = {"workload": "non_max_suppression on %d candidates (%d boxes x %d classes, conf_thres 0, iou 0.5)" % (n * nc, n, nc),
           "ms_per_call": t * 1e3, "detections": int(det[0].shape[0]),
           "reference_ms_per_call_build_container": (ref.get("seconds_per_call") or 0) * 1e3 or None,
           "reference_detections": ref.get("detections"),
           "note": "reference = its own non_max_suppression compiled from source with torchvision.ops.nms restated in numpy "
                   "(torchvision is absent everywhere here): an upper bound on the reference's time, build-container host"}
    if ref.get("seconds_per_call"):
        rec["x_reference"] = ref["seconds_per_call"] / t
    return rec


def predict_record(yv, gu):
    """SparseCADGCN.predict (arch:139-356: root pass -> has_object -> child pass) on a Floorplans-sized proposal tree:
    the device path (one H2D, integer sub-graph extraction kernels, two HIP forwards) next to the loop it replaces —
    the oracle's restatement of the reference's Python o2n / per-edge loops driving the same CPU model."""
    from oracle import oracle_torch as orc
    optkw = dict(n_classes=17, n_blocks=2, n_blocks_out=2)
    data, slices = yv.synth_batch(1, 11, num_proposals=2000, nodes_lo=4, nodes_hi=40, edge_factor=1.2, with_roots=True)
    model = gu.fill_state_(yv.SparseCADGCN(yv.Opt(**optkw)), 0).cuda().eval()

    def one():
        with torch.no_grad():
            return model.predict(data, slices)

    lat, n = _timed_loop(one, 2.0, lo=5, hi=100, warm=3)
    rec = {"workload": "predict(): two-pass inference on one Floorplans-sized item", "proposals": int(data.bbox.shape[0]),
           "nodes": int(data.x.shape[0]), "edges": int(data.edge.shape[0]), "roots": len(data.roots),
           "calls_timed": n, "ms_per_call": lat * 1e3, "items_per_sec": 1.0 / lat}
    ref = gu.fill_state_(orc.SparseCADGCN(orc.Opt(**optkw)), 0).eval()
    cdata, cslices = yv.synth_batch(1, 11, num_proposals=2000, nodes_lo=4, nodes_hi=40, edge_factor=1.2, with_roots=True)
    torch.set_num_threads(min(32, os.cpu_count() or 1))
    with torch.no_grad():
        ref.predict(cdata, cslices)
        t0 = time.perf_counter()
        ref.predict(cdata, cslices)
        tc = time.perf_counter() - t0
    rec["cpu_loop_ms_per_call"] = tc * 1e3
    rec["speedup_vs_cpu_loop"] = tc / lat
    rec["cpu_note"] = "oracle_torch.SparseCADGCN.predict: the reference's Python re-indexing loops + the CPU model"
    return rec


def single_rank_nccl_dp_record(yv, gu, steps=10):
    """The data-parallel step with its RCCL exchange FORCED ON in a process group of one rank: the two asynchronous
    SUM all-reduces (the first fired from inside the backward) run over librccl on this GPU, so the stream ordering
    between the HIP kernels and the collective stream is the multi-GPU one; the result must equal the local step."""
    import torch.distributed as dist
    created = False
    if not dist.is_initialized():
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", str(29500 + os.getpid() % 2000))
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", torch.cuda.current_device()))
        created = True
    try:
        data, slices, optkw, n_graphs = yv.config("4")
        opt = yv.Opt(**optkw)
        to_device(data)
        out = {}
        params = {}
        for mode in ("nccl_exchange", "local"):
            model = gu.fill_state_(yv.SparseCADGCN(opt), 0).cuda()
            # exchange_premul = 2: the buckets are doubled before their all-reduce and halved by Adam (exact), so that
            # `bit_identical_to_local_step` can only hold if every gradient was in its bucket when the exchange was
            # issued — SUM over one rank alone is the identity and would hide a missing join (tests/test_gpu_dist.py)
            tr = yv.Trainer(model, opt, lr=2.5e-4, weight_decay=1e-5, force_exchange=(mode == "nccl_exchange"),
                            exchange_premul=(2.0 if mode == "nccl_exchange" else None))

            def step():
                data._yolat_stage = None
                return tr.step(data, slices)
            for _ in range(3):
                step()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                step()
            torch.cuda.synchronize()
            out[mode] = (time.perf_counter() - t0) / steps
            params[mode] = tr.flat.param.clone()
        g = torch.zeros(1614614, device="cuda")
        for _ in range(3):
            dist.all_reduce(g)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(20):
            dist.all_reduce(g)
        torch.cuda.synchronize()
        t_ar = (time.perf_counter() - t0) / 20
        return {"workload": "cfg4 train step with the gradient exchange forced on, world_size 1",
                "ms_per_step": out["nccl_exchange"] * 1e3, "ms_per_step_without_exchange": out["local"] * 1e3,
                "graphs_per_sec": n_graphs / out["nccl_exchange"],
                "bit_identical_to_local_step": bool(torch.equal(params["nccl_exchange"], params["local"])),
                "exchange_is_identity": False,
                "exchange_note": "buckets x2 on the compute stream before each all-reduce, Adam grad_scale 1/2",
                "allreduce_alone_ms": t_ar * 1e3,
                "collective": "2 async SUM all-reduces per step (fusion+classifier bucket during the conv backward, "
                              "conv bucket after it) over %s" % dist.get_backend()}
    finally:
        if created:
            dist.destroy_process_group()


def participation_record(ms_local, world):
    """What makes an N > 1 line self-verifying: `ranks_seen` = a SUM all-reduce of ones over the collective backend (= N only
    if N ranks took part in the same group), every rank's OWN ms/step (all-gather), its device and host, the backend and
    the RCCL version."""
    import socket
    import torch.distributed as dist
    dev = "cuda" if dist.get_backend() == "nccl" else "cpu"
    ones = torch.ones(1, dtype=torch.float64, device=dev)
    dist.all_reduce(ones, op=dist.ReduceOp.SUM)
    mine = torch.tensor([ms_local], dtype=torch.float64, device=dev)
    gathered = [torch.zeros_like(mine) for _ in range(world)]
    dist.all_gather(gathered, mine)
    ids = [None] * world
    me = {"rank": dist.get_rank(), "host": socket.gethostname(),
          "device": (torch.cuda.current_device() if torch.cuda.is_available() else None),
          "device_name": (torch.cuda.get_device_name() if torch.cuda.is_available() else None)}
    dist.all_gather_object(ids, me)
    try:
        ver = ".".join(str(v) for v in torch.cuda.nccl.version()) if dist.get_backend() == "nccl" else None
    except Exception:
        ver = None
    return {"ranks_seen": int(round(float(ones.item()))), "world_size": world, "backend": dist.get_backend(),
            "rccl_version": ver, "per_rank_ms_per_step": [round(float(t.item()), 5) for t in gathered], "ranks": ids}


def train_dp_record(yv, gu, rank, world, steps, warmup):
    """BASELINE.json configs[3]: Diagrams-style batches of 32 graphs per rank (K = 22), one training step = forward +
    CE + backward + RCCL all-reduce of the flat gradient (two async buckets overlapping the conv backward) + Adam.
    Every rank runs `steps` timed steps between barriers; time = max over ranks.  Also timed: the same step with the
    collective switched off (what the exchange costs after overlap) and the all-reduce of the flat buffer alone."""
    import torch.distributed as dist
    data, slices, optkw, n_graphs = yv.config("4", rank=rank)
    opt = yv.Opt(**optkw)
    model = gu.fill_state_(yv.SparseCADGCN(opt), 0).cuda()
    to_device(data)
    trainer = yv.Trainer(model, opt, lr=2.5e-4, weight_decay=1e-5)

    own = {}

    def timed(fn, n, name=None):
        dist.barrier()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        torch.cuda.synchronize()
        t_own = time.perf_counter() - t0              # this rank's own time, before it waits for the others
        dist.barrier()
        t = torch.tensor([time.perf_counter() - t0], dtype=torch.float64, device="cuda")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        if name:
            own[name] = t_own / n * 1e3
        return float(t.item()) / n

    def step():
        data._yolat_stage = None
        return trainer.step(data, slices)

    for _ in range(max(warmup, 3)):
        step()
    t_step = timed(step, steps, "step")
    # the same step with ONE all-reduce of the whole flat gradient after the backward (YOLAT_DP_BUCKETS=1: fewer, larger
    # collectives — xGMI rings are per-link bound), every rank in the same order
    os.environ["YOLAT_DP_BUCKETS"] = "1"
    try:
        for _ in range(2):
            step()
        t_one = timed(step, steps)
    finally:
        os.environ.pop("YOLAT_DP_BUCKETS", None)
    trainer.exchange_gradients = False
    for _ in range(2):
        step()
    t_local = timed(step, steps)
    trainer.exchange_gradients = True
    broadcast = getattr(yv, "broadcast_parameters")
    broadcast(trainer.flat, model)              # the replicas diverged while the exchange was off
    g = trainer.flat.grad
    for _ in range(3):
        dist.all_reduce(g, op=dist.ReduceOp.SUM)
    t_ar = timed(lambda: dist.all_reduce(g, op=dist.ReduceOp.SUM), max(steps, 20))
    nbytes = g.numel() * 4
    return {"workload": "cfg4 train step (fwd+CE+bwd+all-reduce+Adam), %d Diagrams-style graphs/rank/step, K=%d" %
                        (n_graphs, optkw["n_classes"]),
            "nodes_rank0": int(data.x.shape[0]), "edges_rank0": int(data.edge.shape[0]),
            "proposals_rank0": int(data.bbox.shape[0]), "ms_per_step": t_step * 1e3,
            "graphs_per_sec": n_graphs * world / t_step, "ms_per_step_without_exchange": t_local * 1e3,
            "exchange_cost_ms_after_overlap": (t_step - t_local) * 1e3, "allreduce_bytes": nbytes,
            "ms_per_step_one_bucket": t_one * 1e3, "exchange_cost_ms_one_bucket": (t_one - t_local) * 1e3,
            "steps_through_yolat_train_step": trainer.plan_steps,
            "allreduce_alone_ms": t_ar * 1e3, "allreduce_alone_GBs": nbytes / t_ar / 1e9, "steps": steps,
            "collective": "2 async SUM all-reduces per step (fusion+classifier bucket during the conv backward, conv "
                          "bucket after it) over %s" % dist.get_backend(),
            "participation": participation_record(own["step"], world)}


def main():
    args = parse()
    # stdout carries exactly ONE line, the JSON record: native libraries print banners to fd 1 (RCCL writes its version
    # block there when a communicator is created), so fd 1 points at stderr for the whole run and the record is written
    # to a private duplicate of the real stdout at the end
    sys.stdout.flush()
    real_stdout = os.dup(1)
    os.dup2(2, 1)
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus and world > 1:
        raise SystemExit("--gpus %d but WORLD_SIZE=%d" % (args.gpus, world))
    # YOLAT_BENCH_DEVICE / YOLAT_BENCH_BACKEND exist only so the N>1 control flow can be exercised on a
    # one-GPU box (both ranks on cuda:0 over gloo); the driver's multi-GPU runs use one GPU per rank over RCCL.
    dev_index = int(os.environ.get("YOLAT_BENCH_DEVICE", local))
    torch.cuda.set_device(dev_index)
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        backend = os.environ.get("YOLAT_BENCH_BACKEND", "nccl")        # "nccl" is RCCL on ROCm
        if backend == "nccl":
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", dev_index))
        else:
            dist.init_process_group(backend, rank=rank, world_size=world)

    import yolat_vectorgraphicsrecognition_amd as yv
    sys.path.insert(0, os.path.join(REPO, "tests"))
    import golden_util as gu
    if args.no_side_stream:
        yv.engine.SIDE_STREAM = False

    cfg = args.config or ("2" if args.mode == "fwd" else "3")
    data, slices, optkw, n_graphs = yv.config(cfg, rank=rank)
    N, E, P = data.x.shape[0], data.edge.shape[0], data.bbox.shape[0]
    opt = yv.Opt(**optkw)
    model = gu.fill_state_(yv.SparseCADGCN(opt), 0).cuda()
    to_device(data)

    # forwards in flight: never more than steps/16, so that the fill / drain of the stream pipeline stays a small
    # part of the timed region (with K < 16 steps every step is timed one at a time)
    n_streams = max(1, min(args.streams, args.steps // 16)) if args.mode == "fwd" else 1
    if args.mode == "fwd":
        model.eval()
        model.set_eval_precision(args.precision)
        streams = [torch.cuda.Stream() for _ in range(n_streams)] if n_streams > 1 else [torch.cuda.current_stream()]
        counter = [0]

        def step_on(stream):
            if not args.keep_csr:
                data._yolat_stage = None          # rebuild CSR / segments from the raw COO list
            with torch.cuda.stream(stream), torch.no_grad():
                return model(data, slices)

        def step():
            # every step is one complete forward (COO -> CSR -> ... -> logits) of one graph; consecutive
            # steps go to different streams so that independent forwards overlap on the GPU
            counter[0] += 1
            return step_on(streams[counter[0] % n_streams])

        def step_single():
            return step_on(streams[0])
    else:
        trainer = yv.Trainer(model, opt, lr=2.5e-4, weight_decay=1e-5, precision=args.precision)

        def step():
            data._yolat_stage = None
            return trainer.step(data, slices)

    def barrier():
        if world > 1:
            torch.distributed.barrier()
        torch.cuda.synchronize()

    use_graphs = args.mode == "fwd" and args.graphs
    if use_graphs:
        model.use_hip_graphs(True)        # throughput phase: every stream's plan captures once, then replays
    # one-time setup outside the W warmup steps: every stream's plan folds the BatchNorms, splits / packs the conv
    # weights and allocates its workspace on its first forward (and captures its graph on the second with --graphs)
    for _ in range((3 if use_graphs else 2) * n_streams):
        step()
    for _ in range(args.warmup):
        step()
    barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        last = step()
    barrier()
    elapsed = time.perf_counter() - t0
    dist_proof = None
    if world > 1:
        dist_proof = participation_record(elapsed / args.steps * 1e3, world)      # every rank's own time, before the MAX
        t = torch.tensor([elapsed], dtype=torch.float64, device="cuda")
        torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.MAX)
        elapsed = float(t.item())
    if args.dump_outputs and rank == 0:
        # before any further step: an eval plan's output may live in its stream's workspace
        if args.mode == "fwd":
            dump_outputs(args.dump_outputs, {"pred_cls": last[0], "bbox": last[1]})
        else:
            outs = {"loss": last}
            outs.update(("param." + k, p) for k, p in model.named_parameters())
            dump_outputs(args.dump_outputs, outs)

    # everything below the headline runs with --full only
    full = args.full
    roofline = full and not args.no_roofline
    extras = full and not args.no_extras

    if use_graphs:
        model.use_hip_graphs(False)       # latency / per-stage profiling below use direct launches
    latency_ms = None
    if args.mode == "fwd" and full:
        # ms/forward: latency of ONE forward with nothing else in flight (single stream)
        nlat = min(args.steps, 100)
        for _ in range(5):
            step_single()
        barrier()
        t1 = time.perf_counter()
        for _ in range(nlat):
            step_single()
        torch.cuda.synchronize()
        latency_ms = (time.perf_counter() - t1) / nlat * 1e3

    h2d_inclusive = None
    csr_mode = None
    coo_loader = None
    if args.mode == "fwd" and rank == 0 and full:
        # PCIe-inclusive rate (never `value`): the batch starts as CPU tensors, goes through
        # data.collate_to_device (one pinned staging buffer, one async H2D copy, offset fix-up on the device)
        # and one forward; one batch at a time.
        cpu_item, _, _, _ = yv.config(cfg, rank=rank)
        for k in ("roots",):
            if hasattr(cpu_item, k):
                delattr(cpu_item, k)
        # median of five runs of 100 hand-overs after 20 untimed ones, whatever --steps is (~0.1 s): the loop is bound by
        # the host (collate + enqueue), so a single short run mostly measured allocator warm-up and host noise
        def handover_rate(csr):
            def run(n):
                for _ in range(n):
                    b, sl = yv.collate_to_device([cpu_item], csr=csr)
                    with torch.no_grad():
                        model(b, sl)
                torch.cuda.synchronize()
            run(20)
            rates = []
            for _ in range(5):
                t2 = time.perf_counter()
                run(100)
                rates.append(n_graphs * 100 / (time.perf_counter() - t2))
            return sorted(rates)[2]
        nh = 200
        h2d_inclusive = handover_rate(False)
        # the same with the item's destination-sorted form cached on the item (data.item_csr: computed once per dataset
        # item by the library's host code) and merged into the batch's by offset-add at collate time (csr=True): the
        # forward skips the COO -> CSR conversion, the staging buffer carries int32 CSR arrays instead of int64 COO
        h2d_csr = handover_rate(True)

        # the same hand-over OFF this thread: data.DeviceLoader (csrc/loader.hip: native worker thread, ring of pinned /
        # device slots, copy stream + events) collates and copies batch i + 1 while batch i's forward is enqueued and runs
        # nstreams > 1: consecutive batches are drawn and consumed under different streams (the loader hands a slot back
        # behind an event on the stream its batch was drawn on), so forwards of consecutive batches overlap on the GPU the
        # way `multi_stream` overlaps resident ones — and the hand-over (cold operands, the event packets between
        # forwards: ~6 + 3 us of a one-stream hand-over by kernel trace) hides behind them
        def loader_rate(nstreams=1, csr=True):
            streams = [torch.cuda.Stream() for _ in range(nstreams)] if nstreams > 1 else None

            def run(n):
                loader = yv.DeviceLoader(([cpu_item] for _ in range(n)), slots=nstreams + 2, csr=csr)
                try:
                    with torch.no_grad():
                        k = 0
                        if streams:
                            torch.cuda.set_stream(streams[0])
                        for b, sl in loader:
                            model(b, sl)
                            k += 1
                            if streams:
                                torch.cuda.set_stream(streams[k % nstreams])
                finally:
                    if streams:
                        torch.cuda.set_stream(torch.cuda.default_stream())
                torch.cuda.synchronize()
                loader.close()
            run(60)
            rates = []
            for _ in range(5):
                t2 = time.perf_counter()
                run(300)
                rates.append(n_graphs * 300 / (time.perf_counter() - t2))
            return sorted(rates)[2]
        h2d_loader = loader_rate()
        h2d_loader3 = loader_rate(3)
        # COO mode through the loader (raw index tensors, fix-up by the native worker, CSR rebuilt on the device by every
        # forward = the headline's work per graph) against the one-stream resident rate of that work
        h2d_loader_coo = loader_rate(1, csr=False)
        # merged mode with the batch resident: one forward at a time on the prepared graph
        b, sl = yv.collate_to_device([cpu_item], csr=True)
        for _ in range(5):
            with torch.no_grad():
                model(b, sl)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        for _ in range(nh):
            with torch.no_grad():
                model(b, sl)
        torch.cuda.synchronize()
        merged_ms = (time.perf_counter() - t2) / nh * 1e3
        coo_loader = {"h2d_inclusive_graphs_per_sec_device_loader": h2d_loader_coo,
                      "resident_one_stream_graphs_per_sec": n_graphs / (latency_ms * 1e-3) if latency_ms else None,
                      "device_loader_over_resident_one_stream": h2d_loader_coo * latency_ms * 1e-3 / n_graphs if latency_ms else None}
        csr_mode = {"h2d_inclusive_graphs_per_sec": h2d_csr, "h2d_inclusive_graphs_per_sec_device_loader": h2d_loader,
                    "h2d_inclusive_graphs_per_sec_device_loader_3_streams": h2d_loader3,
                    "ms_per_forward_resident": merged_ms,
                    "device_loader_over_resident_one_stream": h2d_loader * merged_ms * 1e-3 / n_graphs,
                    "device_loader_3_streams_over_resident_one_stream": h2d_loader3 * merged_ms * 1e-3 / n_graphs,
                    "note": "per-item CSR cached on the dataset item (host, once), merged by offset-add at collate "
                            "(yolat_collate_csr_pack), forward on the prepared graph (yolat_forward_eval_csr); the "
                            "headline keeps csr_rebuilt_each_step = true"}

    roof = None
    op_table = None
    nprof = min(args.steps, 50)
    if args.mode == "train" and world > 1 and rank != 0 and roofline:
        for _ in range(nprof):           # the train step contains a collective: every rank must take part
            step()                       # in rank 0's profiling steps
    if rank == 0 and roofline:
        if args.mode == "fwd":
            op_table = plan_profile(step_single, nprof)
        else:
            with OpTimer(yv.ops) as timer:
                for _ in range(nprof):
                    step()
                op_table = timer.summary()
        roof = roofline_entry(op_table, str(cfg) if args.mode == "fwd" else None, args.precision, (N, E, P))
        roof["note"] = ("dominant op by HIP-event time inside this run; algorithmic flops/bytes per launch in "
                        "DESIGN.md; traffic: from the committed separate --pmc passes (null when none exists for "
                        "this workload)")

    agg = edge_roof = fusion_roof = None
    if rank == 0 and roofline:
        agg = aggregation_roofline()
        edge_roof = edge_layer_roofline()
        if op_table is not None and args.mode == "fwd":
            fusion_roof = fusion_stage_roofline(op_table, str(cfg), args.precision)

    cpu = None
    if rank == 0 and world == 1 and full and not args.no_cpu_baseline:      # reported at N=1 only
        cpu = cpu_baseline(cfg, optkw, args.mode)

    multi = floor = train_dp = None
    if args.mode == "fwd" and rank == 0 and extras:
        # serving-style throughput with many forwards in flight, over >= 512 forwards whatever --steps is
        multi = multi_stream_throughput(model, data, slices, n_graphs, n_streams=max(args.streams, 1),
                                        forwards=1024 if (N < 50000) else 256, keep_csr=args.keep_csr)
        if world == 1 and str(cfg) == "2" and args.precision == "fp32":
            floor = floorplans_sized_record(yv, gu, cpu=not args.no_cpu_baseline)
    more = {}
    if rank == 0 and world == 1 and extras and args.mode == "fwd" and str(cfg) == "2" \
            and args.precision == "fp32":
        # the other BASELINE.json configurations, bounded to a few seconds each, so that the driver's N = 1 line
        # carries them: configs[2] (cfg 3 train step), configs[4] (cfg 5, fp32 and bf16 storage), predict(), and the
        # data-parallel step with its RCCL exchange forced on in a one-rank group
        torch.cuda.empty_cache()

        def guarded(name, fn):
            try:
                more[name] = fn()
            except Exception as exc:                          # a sub-record must never cost the headline line
                more[name] = {"error": "%s: %s" % (type(exc).__name__, exc)}
            torch.cuda.empty_cache()

        guarded("train_cfg3", lambda: train_config_record(yv, gu, "3", cpu=not args.no_cpu_baseline))
        guarded("cfg5_fp32", lambda: eval_config_record(yv, gu, "5", "fp32"))
        guarded("cfg5_bf16", lambda: eval_config_record(yv, gu, "5", "bf16"))
        guarded("train_cfg5_fp32", lambda: train_config_record(yv, gu, "5", "fp32", budget_s=3.0, cpu=False))
        guarded("train_cfg5_bf16", lambda: train_config_record(yv, gu, "5", "bf16", budget_s=3.0, cpu=False))
        guarded("predict", lambda: predict_record(yv, gu))
        guarded("proposals", lambda: proposals_record(yv))
        guarded("nms", lambda: nms_record(yv))
        guarded("train_dp_single_rank_nccl", lambda: single_rank_nccl_dp_record(yv, gu))
    if world > 1 and extras:
        # the data-parallel training step (north_star: RCCL all-reduce of gradients over xGMI) next to the replicas
        train_dp = train_dp_record(yv, gu, rank, world, steps=max(min(args.steps, 50), 10), warmup=args.warmup)

    if world > 1:
        torch.distributed.barrier()
    if rank == 0:
        ms = elapsed / args.steps * 1e3
        line = {
            "metric": "graphs_per_sec" if args.mode == "fwd" else "train_graphs_per_sec",
            "value": n_graphs * world * args.steps / elapsed,
            "unit": "graphs/s",
            "n_gpus": world,
            "participation": dist_proof,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": ms,
            "ms_per_forward": latency_ms,
            "h2d_inclusive_graphs_per_sec": h2d_inclusive,
            "csr_merged_mode": csr_mode,
            "coo_mode_device_loader": coo_loader,
            "single_stream_graphs_per_sec": (n_graphs * world / (latency_ms * 1e-3)) if latency_ms else None,
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": "f32" if args.precision == "fp32" else "bf16 storage / f32 accumulate",
            "data": "synthetic",
            "config": {"workload": "cfg%s %s: synthetic Bezier graph(s), in_channels=5, n_blocks=%d, "
                                   "%d graph(s)/rank/step" % (cfg, "eval forward" if args.mode == "fwd"
                                                              else "train step (fwd+CE+bwd+Adam)",
                                                              optkw["n_blocks"], n_graphs),
                       "nodes": N, "edges": E, "proposals": P, "n_classes": optkw["n_classes"],
                       "csr_rebuilt_each_step": not args.keep_csr, "precision": args.precision,
                       "streams_in_flight": n_streams, "hip_graph_replay": bool(args.mode == "fwd" and args.graphs),
                       "parallelism": "replicas (graph-id sharding)" if args.mode == "fwd" else "dp%d" % world},
            "multi_stream": multi,
            "floorplans_sized": floor,
            "train_dp": train_dp,
            "roofline": roof,
            "roofline_aggregation": agg,
            "roofline_edge_layer": edge_roof,
            "roofline_fusion": fusion_roof,
            "cpu_baseline": cpu,
        }
        line.update(more)
        in_step = pick_path(more, "train_cfg5_fp32", "csr_mean_fwd_us_per_call_in_step")
        if agg is not None:
            # the same kernel on the same graph inside the cfg-5 fp32 training step (cold operands, neighbours in flight) runs
            # slower than back to back on its own: `frac` quotes the IN-STEP time when this run has it, the stand-alone
            # figure stays beside it
            agg["frac_standalone"] = agg["frac"]
            agg["avg_launch_us_standalone"] = agg["avg_launch_us"]
            agg["in_step_us"] = in_step
            if in_step:
                agg["achieved"] = agg["bytes_per_launch"] / (in_step * 1e-6) / 1e9
                agg["frac"] = agg["achieved"] / PEAK_HBM_GBS
                agg["avg_launch_us"] = in_step
                agg["quoted_on"] = "median call inside the cfg-5 fp32 training step (train_cfg5_fp32 op table)"
            else:
                agg["quoted_on"] = "stand-alone loop (no training leg in this run)"
        if op_table is not None:
            top = sorted(op_table.items(), key=lambda kv: -kv[1]["ms_total"])[:6]
            line["op_breakdown_us"] = {k: round(v["ms_total"] / max(min(args.steps, 50), 1) * 1e3, 2) for k, v in top}
            line["gpu_us_per_step_sum_of_stages"] = round(sum(v["ms_total"] for v in op_table.values()) /
                                                          max(min(args.steps, 50), 1) * 1e3, 1)
        # flat scalars of every sub-record as the LAST ~600 characters of the line (the driver keeps the line's tail)
        def pick(d, *path):
            for k in path:
                if not isinstance(d, dict) or k not in d or d[k] is None:
                    return None
                d = d[k]
            return round(d, 4) if isinstance(d, float) else d
        line["summary"] = {
            "graphs_per_sec": round(line["value"], 1), "ms_per_forward": pick(line, "ms_per_forward"),
            "train_cfg3_ms": pick(line, "train_cfg3", "ms_per_step"),
            "train_cfg3_host_ms": pick(line, "train_cfg3", "one_call_plan", "host_ms_per_step"), "cfg5_fp32_ms": pick(line, "cfg5_fp32", "ms_per_forward"),
            "cfg5_bf16_ms": pick(line, "cfg5_bf16", "ms_per_forward"),
            "train_cfg5_fp32_ms": pick(line, "train_cfg5_fp32", "ms_per_step"),
            "train_cfg5_bf16_ms": pick(line, "train_cfg5_bf16", "ms_per_step"),
            "csr_merged_ms": pick(line, "csr_merged_mode", "ms_per_forward_resident"),
            "csr_merged_h2d_gps": pick(line, "csr_merged_mode", "h2d_inclusive_graphs_per_sec"),
            "loader_h2d_gps": pick(line, "csr_merged_mode", "h2d_inclusive_graphs_per_sec_device_loader"),
            "loader3_h2d_gps": pick(line, "csr_merged_mode", "h2d_inclusive_graphs_per_sec_device_loader_3_streams"),
            "loader_coo_h2d_gps": pick(line, "coo_mode_device_loader", "h2d_inclusive_graphs_per_sec_device_loader"),
            "loader_coo_over_resident": pick(line, "coo_mode_device_loader", "device_loader_over_resident_one_stream"),
            "h2d_inclusive_gps": pick(line, "h2d_inclusive_graphs_per_sec"), "multi_stream_gps": pick(line, "multi_stream", "value"),
            "floorplans_ms": pick(line, "floorplans_sized", "ms_per_forward"),
            "floorplans_x_cpu": pick(line, "floorplans_sized", "speedup_vs_cpu_one_at_a_time"),
            "predict_ms": pick(line, "predict", "ms_per_call"), "proposals_ms": pick(line, "proposals", "ms_per_svg"),
            "nms_ms": pick(line, "nms", "ms_per_call"), "dp1_nccl_ms": pick(line, "train_dp_single_rank_nccl", "ms_per_step"),
            "dp1_bit_identical": pick(line, "train_dp_single_rank_nccl", "bit_identical_to_local_step"),
            "cpu_gps": pick(line, "cpu_baseline", "value"), "roofline_frac": pick(line, "roofline", "frac"),
            "roofline_frac_executed": pick(line, "roofline", "frac_executed_pipe"),
            "agg_hbm_frac": pick(line, "roofline_aggregation", "frac")}
        sys.stdout.flush()
        os.write(real_stdout, (json.dumps(line) + "\n").encode())
    if world > 1:
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
