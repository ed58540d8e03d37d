"""Launch helpers of the GPU tests of the one-launch proposal-local conv stack (csrc/conv_local.hip), shared by
tests/test_gpu_conv_local.py and tests/test_gpu_conv_local_elements.py.  Imports the extension lazily (GPU tests only)."""
import ctypes
import os

import torch


class _mode(object):
    """YOLAT_CONV_LOCAL for the duration of a block (read per call by yolat_forward_eval_bf16)."""

    def __init__(self, v):
        self.v = str(v)

    def __enter__(self):
        self.old = os.environ.get("YOLAT_CONV_LOCAL")
        os.environ["YOLAT_CONV_LOCAL"] = self.v

    def __exit__(self, *a):
        if self.old is None:
            os.environ.pop("YOLAT_CONV_LOCAL", None)
        else:
            os.environ["YOLAT_CONV_LOCAL"] = self.old


def _run_stack(yv, model, d, warm=True):
    """yolat_conv_stack_local_bf16 on the model's packed weights: (feats [N,D] bf16, Z [P, 2(F+D)] fp32, flag).
    warm=False: the model's plan exists already (a forward has run) and `d` is not sent through the whole forward."""
    from yolat_vectorgraphicsrecognition_amd import ops
    from yolat_vectorgraphicsrecognition_amd._lib import lib, check, GraphCsr
    if warm:
        with torch.no_grad():
            model(d, None)                  # builds the plan (weights folded / packed)
    plan = model._yolat_plan
    h = plan._desc_h
    assert h is not None and h.conv_local, "the plan did not pack the conv stack"
    base = plan._desc
    N, P = d.x.shape[0], d.bbox.shape[0]
    dev = torch.device("cuda")
    g = ops.build_graph(d.edge.to(dev), d.e_attr.to(dev), d.bbox_idx.to(dev), N, P)
    g.check_status()
    D, F = base.C * base.n_blocks_out, base.F
    feats = torch.full((N, D), float("nan"), dtype=torch.bfloat16, device=dev)
    Z = torch.full((P, 2 * (F + D)), float("nan"), dtype=torch.float32, device=dev)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    x = d.x.to(dev).contiguous()
    gc = GraphCsr(*g.device_pointers())
    check(lib.yolat_conv_stack_local_bf16(ctypes.byref(h), h.conv_local, x.data_ptr(), x.stride(0), ctypes.byref(gc), N, g.E,
                                          P, feats.data_ptr(), D, Z.data_ptr(), Z.stride(0), flag.data_ptr(),
                                          torch.cuda.current_stream().cuda_stream), "yolat_conv_stack_local_bf16")
    torch.cuda.synchronize()
    return feats, Z, int(flag.item()), (F, D)


def _run_stack_coo(yv, model, d, warm=True):
    """yolat_conv_stack_local_bf16_coo on the raw edge list: (feats, Z, flag, status)"""
    from yolat_vectorgraphicsrecognition_amd._lib import lib, check
    if warm:
        with torch.no_grad():
            model(d, None)
    plan = model._yolat_plan
    h, base = plan._desc_h, plan._desc
    N, P, E = d.x.shape[0], d.bbox.shape[0], d.edge.shape[0]
    dev = torch.device("cuda")
    D, F = base.C * base.n_blocks_out, base.F
    feats = torch.full((N, D), float("nan"), dtype=torch.bfloat16, device=dev)
    Z = torch.full((P, 2 * (F + D)), float("nan"), dtype=torch.float32, device=dev)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    x, edge, attr, bb = d.x.to(dev).contiguous(), d.edge.to(dev), d.e_attr.to(dev).contiguous(), d.bbox_idx.to(dev)
    need = int(lib.yolat_batch_locality_workspace_bytes(N, E, P))
    ws = torch.empty(need + 16, dtype=torch.uint8, device=dev)
    check(lib.yolat_conv_stack_local_bf16_coo(ctypes.byref(h), h.conv_local, x.data_ptr(), x.stride(0), edge.data_ptr(),
                                              edge.stride(0), edge.stride(1), attr.data_ptr(), bb.data_ptr(), N, E, P,
                                              feats.data_ptr(), D, Z.data_ptr(), Z.stride(0), flag.data_ptr(),
                                              status.data_ptr(), ws.data_ptr(), ws.numel(),
                                              torch.cuda.current_stream().cuda_stream), "yolat_conv_stack_local_bf16_coo")
    torch.cuda.synchronize()
    return feats, Z, int(flag.item()), int(status.item()), (F, D)


def tune(nw, g0=0):
    """waves per workgroup (4 | 8, 0 = automatic) and proposals per workgroup (0 = automatic) of the next launches"""
    from yolat_vectorgraphicsrecognition_amd._lib import lib
    lib.yolat_conv_local_tune(int(nw), int(g0), 0, None)


def to_data(yv, lay, x, e_attr):
    """a plain Data from a layout's arrays (tests/conv_local_ref.py: layout, inputs)"""
    P = lay["P"]
    d = yv.Data(x=x.clone(), pos=x[:, :2].clone())
    d.edge = torch.from_numpy(lay["edge"].copy())
    d.e_attr = e_attr.clone()
    d.bbox_idx = torch.from_numpy(lay["bbox_idx"].copy())
    d.bbox = torch.zeros(P, 4)
    d.stat_feats = torch.zeros(P, 13)
    d.labels = torch.zeros(P, dtype=torch.int64)
    d.is_super = torch.zeros(x.shape[0], dtype=torch.bool)
    return d


def _at(plan, ptr, n, dtype):
    """the n elements of `dtype` at device address ptr, found inside the tensors the plan keeps alive (its folds) or the
    model's own parameters and buffers — the descriptor holds addresses only"""
    ptr = int(ptr or 0)
    assert ptr, "null operand in the descriptor"
    size = torch.empty(0, dtype=dtype).element_size()
    for t in list(plan._keep) + list(plan._tensors):
        lo = t.data_ptr()
        if lo <= ptr and ptr + n * size <= lo + t.numel() * t.element_size() and t.is_contiguous():
            flat = t.detach().reshape(-1).view(torch.uint8)[ptr - lo:ptr - lo + n * size]
            return flat.cpu().clone().view(dtype)
    raise AssertionError("descriptor address %#x is not inside any tensor of the plan" % ptr)


def plan_operands(plan):
    """The folded operands of every conv layer READ BACK from the plan's descriptors (what k_conv_local_pack was given),
    as CPU tensors in the form of conv_local_ref.fold_state."""
    d, h = plan._desc, plan._desc_h
    C = int(d.C)
    out = []
    for l in range(int(d.n_blocks)):
        c = d.conv[l]
        cin = int(c.Cin)
        f32 = torch.float32
        out.append(dict(
            Cin=cin, Wuv=_at(plan, c.Wuv, 2 * C * cin, f32).view(2 * C, cin), Wc4=_at(plan, c.Wc4, 4 * C, f32).view(C, 4),
            uv_scale=_at(plan, h.uv_scale[l], 2 * C, f32), uv_shift=_at(plan, h.uv_shift[l], 2 * C, f32),
            s1=_at(plan, c.s1, C, f32), Wr=_at(plan, c.Wr, C * cin, f32).view(C, cin), br=_at(plan, c.br, C, f32),
            Wn=_at(plan, c.Wn, C * cin, f32).view(C, cin), bn=_at(plan, c.bn, C, f32), sn=_at(plan, c.sn, C, f32),
            tn=_at(plan, c.tn, C, f32), W2f=_at(plan, h.W2[l], C * C, torch.bfloat16).view(C, C),
            t2f=_at(plan, h.t2f[l], C, f32)))
    return out
