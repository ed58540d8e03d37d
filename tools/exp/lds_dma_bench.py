"""LDS-DMA experiment: the cfg-2 classifier-1 GEMM (P = 400 rows, 2304 -> 512; k_gemm_nt_sk, 122 MB of
operand tiles through L2 -> CU) with its tiles brought in by global_load_lds_dwordx4 (k_gemm_nt_sk_dma) instead of
global -> VGPR -> ds_write.  Bit-identity check, HIP-event timing of both, in-kernel s_memtime split of the DMA variant
(cycles waiting for the tile / computing), and the cfg-2 forward with either kernel.  Also the bf16x6 variant of the 8-wave
kernel (yolat_linear_sk_x6, csrc/linear_sk_x6.hip): timing, error against fp64 and the same in-kernel split.
usage: python tools/exp/lds_dma_bench.py [reps=200]"""
import ctypes, os, sys, time
import numpy as np
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import yolat_vectorgraphicsrecognition_amd as yv
from yolat_vectorgraphicsrecognition_amd import ops
from yolat_vectorgraphicsrecognition_amd._lib import lib

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 200
hook = lib.yolat_debug_gemm_sk_dma
hook.restype = None
hook.argtypes = [ctypes.c_int, ctypes.c_void_p]
torch.manual_seed(0)
for (M, K, N) in ((400, 2304, 512), (400, 512, 256), (2000, 2304, 512)):
    A = torch.randn(M, K, device="cuda")
    lin = torch.nn.Linear(K, N).cuda()
    Y0, Y1 = torch.empty(M, N, device="cuda"), torch.empty(M, N, device="cuda")

    def run(Y):
        ops.linear_fwd(A, lin.weight.detach(), lin.bias.detach(), Y)

    def timed(Y):
        for _ in range(10):
            run(Y)
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(reps):
            run(Y)
        e.record()
        torch.cuda.synchronize()
        return s.elapsed_time(e) / reps * 1e3
    hook(0, None)
    t0 = timed(Y0)
    hook(4, None)
    t1 = timed(Y1)
    Y8 = torch.empty(M, N, device="cuda")
    hook(8, None)
    t8 = timed(Y8)
    print("   8-wave LDS-DMA variant: %.2f us, max |diff| to the 4-wave result %.3e of scale %.3e" %
          (t8, float((Y8 - Y0).abs().max()), float(Y0.abs().max())))
    grid = ((M + 31) // 32) * ((N + 31) // 32)
    stamps = torch.zeros(3 * grid + 8, dtype=torch.int64, device="cuda")
    hook(8, stamps.data_ptr())
    run(Y1)
    torch.cuda.synchronize()
    hook(0, None)
    st = stamps.cpu().numpy()[:3 * grid].reshape(grid, 3)
    st = st[st[:, 2] > 0]
    # the bf16x6 variant of the 8-wave kernel (csrc/linear_sk_x6.hip, yolat_linear_sk_x6): same tiles, products on the bf16 MFMA
    Y6 = torch.empty(M, N, device="cuda")
    run8, run = run, lambda Y: ops.linear_sk_x6(A, lin.weight.detach(), lin.bias.detach(), Y)
    hook(0, None)
    t6 = timed(Y6)
    stamps6 = torch.zeros(3 * grid + 8, dtype=torch.int64, device="cuda")
    hook(0, stamps6.data_ptr())
    run(Y6)
    torch.cuda.synchronize()
    hook(0, None)
    run = run8
    s6 = stamps6.cpu().numpy()[:3 * grid].reshape(grid, 3)
    s6 = s6[s6[:, 2] > 0]
    ref = (A.double() @ lin.weight.detach().double().t() + lin.bias.detach().double())
    nch = K // 128
    print("   8-wave LDS-DMA bf16x6 variant: %.2f us (fp32 8-wave %.2f us) | max |err| vs fp64: x6 %.3e, fp32 MFMA %.3e of scale %.3e | "
          "per workgroup: waiting for tiles %.0f cycles, reads + split + MFMA %.0f, whole K loop %.0f = %.0f per chunk (fp32 8-wave: "
          "%.0f / %.0f / %.0f = %.0f per chunk)"
          % (t6, t8, float((Y6.double() - ref).abs().max()), float((Y8.double() - ref).abs().max()), float(ref.abs().max()),
             s6[:, 0].mean(), s6[:, 1].mean(), s6[:, 2].mean(), s6[:, 2].mean() / nch,
             st[:, 0].mean(), st[:, 1].mean(), st[:, 2].mean(), st[:, 2].mean() / nch))
    print("M=%d K=%d N=%d (%d workgroups): VGPR-staged %.2f us | LDS-DMA %.2f us | bit-identical %s | 8-wave DMA variant per workgroup: "
          "waiting for tiles %.0f cycles, MFMA + reads %.0f, whole K loop %.0f (%d chunks)"
          % (M, K, N, grid, t0, t1, bool(torch.equal(Y0, Y1)), st[:, 0].mean() if len(st) else -1, st[:, 1].mean() if len(st) else -1,
             st[:, 2].mean() if len(st) else -1, K // 128))

# the cfg-2 forward with either kernel
data, slices, optkw, _ = yv.config("2")
model = yv.SparseCADGCN(yv.Opt(**optkw)).cuda().eval()
x, edge, ea, bb = data.x.cuda(), data.edge.cuda(), data.e_attr.cuda(), data.bbox_idx.cuda()
P = int(data.bbox.shape[0])
with torch.no_grad():
    model(data, slices)
    plan = model._yolat_plan
    res = {}
    for on in (0, 8, 0, 8):
        hook(on, None)
        for _ in range(20):
            out = plan.run(x, edge, ea, bb, P)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(500):
            out = plan.run(x, edge, ea, bb, P)
        torch.cuda.synchronize()
        res.setdefault(on, []).append((time.perf_counter() - t0) / 500 * 1e3)
        res["out%d" % on] = out.clone()
    hook(0, None)
print("cfg-2 forward (one at a time, host clock): VGPR-staged %s ms | LDS-DMA (8 waves) %s ms | logits identical %s"
      % (["%.4f" % t for t in res[0]], ["%.4f" % t for t in res[8]], bool(torch.equal(res["out0"], res["out8"]))))
