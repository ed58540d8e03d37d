"""Tensor-level wrappers of the C ABI (include/yolat_hip.h).

Every function takes torch CUDA tensors, checks dtype / device / inner stride, and enqueues the HIP
kernel(s) on torch's current stream.  torch is used for device memory and streams only — the
arithmetic is in libyolat_hip.so.  There is no CPU path: a non-CUDA tensor raises.
"""
import ctypes
import os

import torch

from ._lib import lib, check

STATS_ROWS = 32
STATUS_EDGE_RANGE, STATUS_SEG_UNSORTED, STATUS_SEG_RANGE, STATUS_NOT_LOCAL = 1, 2, 4, 8

# The HIP kernels write parameters and BatchNorm buffers through raw pointers, which torch's per-tensor `_version`
# counters never see.  Every wrapper below that modifies model state (Adam step, running-statistic updates) bumps
# this epoch; every cache derived from model state (folded eval BatchNorm coefficients in engine._bn_eval, the
# eval plan's descriptor in plan.EvalPlan) carries it in its key.
_WEIGHT_EPOCH = [0]


def weight_epoch():
    return _WEIGHT_EPOCH[0]


def bump_weight_epoch():
    _WEIGHT_EPOCH[0] += 1


_RAW_STREAM = getattr(torch._C, "_cuda_getCurrentRawStream", None)
_GET_DEVICE = getattr(torch._C, "_cuda_getDevice", None)
_STREAM_OBJ = {}


def _stream():
    """Raw handle of the current HIP stream.  (torch.cuda.current_stream() resolves the device through several Python
    layers: ~3 us a call, three calls per forward; the two C entry points are what it ends in.)"""
    if _RAW_STREAM is not None and _GET_DEVICE is not None:
        return _RAW_STREAM(_GET_DEVICE())
    return torch.cuda.current_stream().cuda_stream


def current_stream_object():
    """torch.cuda.Stream object of the current stream, cached per (device, raw handle)."""
    if _RAW_STREAM is None or _GET_DEVICE is None:
        return torch.cuda.current_stream()
    dev = _GET_DEVICE()
    raw = _RAW_STREAM(dev)
    hit = _STREAM_OBJ.get(dev)
    if hit is None or hit[0] != raw:
        hit = _STREAM_OBJ[dev] = (raw, torch.cuda.current_stream())
    return hit[1]


def _f(t, name="tensor", allow_none=False):
    """data_ptr of an fp32 CUDA tensor whose last dim is dense."""
    if t is None:
        if allow_none:
            return None
        raise ValueError("%s is None" % name)
    if not t.is_cuda:
        raise RuntimeError("%s must be a CUDA (ROCm) tensor — the yolat HIP path has no CPU fallback" % name)
    if t.dtype != torch.float32:
        raise TypeError("%s must be float32, got %s" % (name, t.dtype))
    if t.dim() >= 1 and t.shape[-1] > 1 and t.stride(-1) != 1 and t.numel() > 0:      # (an empty tensor's strides mean nothing)
        raise ValueError("%s must be dense along its last dimension" % name)
    return t.data_ptr()


def _h(t, name="tensor"):
    """data_ptr of a bfloat16 CUDA tensor whose last dim is dense (bf16-storage training tensors)."""
    if not t.is_cuda or t.dtype != torch.bfloat16:
        raise TypeError("%s must be a bfloat16 CUDA tensor" % name)
    if t.dim() >= 1 and t.shape[-1] > 1 and t.stride(-1) != 1 and t.numel() > 0:      # (an empty tensor's strides mean nothing)
        raise ValueError("%s must be dense along its last dimension" % name)
    return t.data_ptr()


def _is_h(t):
    return t is not None and t.dtype == torch.bfloat16


def _fh(t, name="tensor", half=None):
    """data_ptr of a tensor stored as bfloat16 or fp32: by its own dtype, or checked against the storage `half` names."""
    return _h(t, name) if (_is_h(t) if half is None else half) else _f(t, name)


def _i(t, dtype, name="index"):
    if t is None:
        return None
    if not t.is_cuda:
        raise RuntimeError("%s must be a CUDA (ROCm) tensor" % name)
    if t.dtype != dtype:
        raise TypeError("%s must be %s, got %s" % (name, dtype, t.dtype))
    if t.dim() == 1 and t.numel() > 1 and t.stride(0) != 1:
        raise ValueError("%s must be contiguous" % name)
    return t.data_ptr()


def _ld(t):
    return t.stride(0) if t.shape[0] > 1 else max(t.shape[-1], t.stride(0))


# ---------------------------------------------------------------------------------------------
# graph pre-processing
# ---------------------------------------------------------------------------------------------

_ZERO_STATUS = {}


def check_status_word(status):
    """Synchronising read of an input-validity word (one int32 the pre-processing kernels OR their STATUS_* flags into):
    raises what the reference raises on such a batch, returns True on zero."""
    s = int(status.item())
    if s & STATUS_EDGE_RANGE:
        raise IndexError("edge_index contains a node id outside [0, N)")
    if s & STATUS_SEG_UNSORTED:
        raise ValueError("bbox_idx is not non-decreasing")
    if s & STATUS_SEG_RANGE:
        raise IndexError("bbox_idx contains a proposal id outside [0, P)")
    if s & STATUS_NOT_LOCAL:
        raise ValueError("a batch handed over as proposal-local (yolat_locality) is not: an edge leaves its proposal, "
                         "the edge list is not grouped by proposal, or a proposal does not fit a tile")
    return True


class Graph(object):
    """Device-resident integer structure of one batch (CSR by destination, optional CSC by source,
    proposal segments).  Owned by the caller / cached on the batch object."""

    __slots__ = ("N", "E", "P", "row_ptr", "perm", "src", "dst", "attr", "col_ptr", "slots",
                 "seg_ptr", "node_seg", "status", "_work", "_inv_deg")

    @classmethod
    def from_arrays(cls, N, E, P, row_ptr, src, dst, attr, seg_ptr, node_seg, perm=None):
        """A Graph over device arrays prepared elsewhere (data.collate_to_device(csr=True): the batch's CSR merged on
        the host from the items' cached CSRs and shipped with the batch).  The ids were validated where the arrays
        were built, so the status word is zero."""
        g = cls()
        g._inv_deg = None
        g.N, g.E, g.P = int(N), int(E), int(P)
        g.row_ptr, g.src, g.dst, g.attr, g.seg_ptr, g.node_seg, g.perm = row_ptr, src, dst, attr, seg_ptr, node_seg, perm
        g.col_ptr = g.slots = None
        g._work = None
        st = _ZERO_STATUS.get(row_ptr.device)          # shared, never written for a prepared graph
        if st is None:
            st = _ZERO_STATUS[row_ptr.device] = torch.zeros(1, dtype=torch.int32, device=row_ptr.device)
        g.status = st
        return g

    def device_pointers(self):
        """(row_ptr, src, dst, attr, seg_ptr, node_seg) device addresses — what yolat_graph_csr carries."""
        return (self.row_ptr.data_ptr(), self.src.data_ptr(), self.dst.data_ptr(), self.attr.data_ptr(),
                self.seg_ptr.data_ptr(), self.node_seg.data_ptr())

    def inv_deg(self):
        """[N] fp32 1 / max(in-degree, 1) (the factor of the mean aggregation's backward), built once per graph."""
        if getattr(self, "_inv_deg", None) is None:
            inv = torch.empty(self.N, dtype=torch.float32, device=self.row_ptr.device)
            check(lib.yolat_inv_degree(self.row_ptr.data_ptr(), self.N, inv.data_ptr(), _stream()), "yolat_inv_degree")
            self._inv_deg = inv
        return self._inv_deg

    def ensure_csc(self):
        if self.col_ptr is None:
            dev = self.row_ptr.device
            self.col_ptr = torch.empty(self.N + 1, dtype=torch.int32, device=dev)
            self.slots = torch.empty(max(self.E, 1), dtype=torch.int32, device=dev)
            work = torch.empty(int(lib.yolat_csc_work_elems(self.N)), dtype=torch.int32, device=dev)
            check(lib.yolat_csc_by_source(self.src.data_ptr(), self.E, self.N, self.col_ptr.data_ptr(),
                                          self.slots.data_ptr(), work.data_ptr(), _stream()),
                  "yolat_csc_by_source")
            self._work = work  # keep alive until the stream has consumed it
        return self

    def check_status(self):
        """Synchronising validity check of the flags raised by the pre-processing kernels."""
        return check_status_word(self.status)


class PackedGraph(Graph):
    """A prepared graph whose six arrays live at known offsets of ONE device buffer (data.collate_to_device(csr=True)):
    the eval forward only needs their addresses (device_pointers), so the tensor views are made on first use — the
    training path and the tests read them — instead of twelve tensor operations per batch."""

    __slots__ = ("_buf", "_offs", "_views")
    _FIELDS = {"row_ptr": 0, "src": 1, "dst": 2, "attr": 3, "seg_ptr": 4, "node_seg": 5}

    @classmethod
    def from_buffer(cls, buf, offs, N, E, P):
        g = cls()
        g._inv_deg = None
        g.N, g.E, g.P = int(N), int(E), int(P)
        g._buf, g._offs, g._views = buf, tuple(int(o) for o in offs), {}
        g.perm = None
        g.col_ptr = g.slots = None
        g._work = None
        st = _ZERO_STATUS.get(buf.device)
        if st is None:
            st = _ZERO_STATUS[buf.device] = torch.zeros(1, dtype=torch.int32, device=buf.device)
        g.status = st
        return g

    def device_pointers(self):
        base = self._buf.data_ptr()
        return tuple(base + o for o in self._offs)

    def _view(self, name):
        v = self._views.get(name)
        if v is None:
            i = self._FIELDS[name]
            Ee = max(self.E, 1)
            shape = ((self.N + 1,), (Ee,), (Ee,), (Ee, 4), (self.P + 1,), (self.N,))[i]
            dtype = torch.float32 if name == "attr" else torch.int32
            n = 1
            for d in shape:
                n *= d
            o = self._offs[i] // 4
            v = self._views[name] = self._buf.view(dtype)[o:o + n].view(shape)
        return v

    row_ptr = property(lambda self: self._view("row_ptr"))
    src = property(lambda self: self._view("src"))
    dst = property(lambda self: self._view("dst"))
    attr = property(lambda self: self._view("attr"))
    seg_ptr = property(lambda self: self._view("seg_ptr"))
    node_seg = property(lambda self: self._view("node_seg"))


def edge_layout(edge):
    """(E, stride_e, stride_c) of an edge list given as [E,2] (data.edge) or as [2,E], its transposed view included: the
    element strides between edges and between the two ends of one.  A [2,2] tensor is [E,2] unless it is a transposed
    view (stride(0) == 1)."""
    if edge.dim() == 2:
        if edge.shape[1] == 2 and not (edge.shape[0] == 2 and edge.stride(0) == 1):
            return edge.shape[0], edge.stride(0), edge.stride(1)
        if edge.shape[0] == 2:
            return edge.shape[1], edge.stride(1), edge.stride(0)
    raise ValueError("edge must be [E,2] or [2,E]")


def build_graph(edge, e_attr, bbox_idx, num_nodes, num_proposals):
    """edge: int64 CUDA tensor, either [E,2] (data.edge) or its [2,E] transposed view;
    e_attr: fp32 [E,4]; bbox_idx: int64 [N] or None."""
    E, se, sc = edge_layout(edge)
    dev = edge.device
    N, P = int(num_nodes), int(num_proposals)
    g = Graph()
    g._inv_deg = None
    g.N, g.E, g.P = N, E, P
    g.col_ptr = g.slots = None
    g.row_ptr = torch.empty(N + 1, dtype=torch.int32, device=dev)
    g.perm = torch.empty(max(E, 1), dtype=torch.int32, device=dev)
    g.src = torch.empty(max(E, 1), dtype=torch.int32, device=dev)
    g.dst = torch.empty(max(E, 1), dtype=torch.int32, device=dev)
    g.attr = torch.empty(max(E, 1), 4, dtype=torch.float32, device=dev)
    g.seg_ptr = g.node_seg = None
    if bbox_idx is not None:
        # zero-initialised: with a malformed (unsorted) bbox_idx the kernels flag STATUS_SEG_UNSORTED and the
        # pointers stay inside [0, N] whatever the write order, so every downstream kernel is memory-safe.
        # (status word, segment pointers and node segments as slices of ONE zeroed buffer: one fill, not three)
        n_seg = (P + 1 + 3) // 4 * 4
        z = torch.zeros(4 + n_seg + max(N, 1), dtype=torch.int32, device=dev)
        g.status = z[0:1]
        g.seg_ptr = z[4:4 + P + 1]
        g.node_seg = z[4 + n_seg:4 + n_seg + max(N, 1)]
    else:
        g.status = torch.zeros(1, dtype=torch.int32, device=dev)
    if E > 0:
        if e_attr.shape[0] != E or e_attr.shape[1] != 4:
            raise ValueError("e_attr must be [E,4]")
        if not e_attr.is_contiguous():
            e_attr = e_attr.contiguous()
    work = torch.empty(int(lib.yolat_graph_work_elems(N, E)), dtype=torch.int32, device=dev)
    check(lib.yolat_graph_prepare(_i(edge, torch.int64, "edge"), se, sc, _f(e_attr, "e_attr") if E > 0 else None,
                                  _i(bbox_idx, torch.int64, "bbox_idx"), E, N, P, g.row_ptr.data_ptr(),
                                  g.perm.data_ptr(), g.src.data_ptr(), g.dst.data_ptr(), g.attr.data_ptr(),
                                  g.seg_ptr.data_ptr() if g.seg_ptr is not None else None,
                                  g.node_seg.data_ptr() if g.node_seg is not None else None,
                                  work.data_ptr(), g.status.data_ptr(), _stream()), "yolat_graph_prepare")
    g._work = work
    return g


def segment_ptr(bbox_idx, num_proposals):
    """[P + 1] int32 node range pointers of a non-decreasing int64 ``bbox_idx`` [N] (yolat_segment_ptr)."""
    P, N = int(num_proposals), int(bbox_idx.shape[0])
    dev = bbox_idx.device
    # zero-initialised, like build_graph's: with an unsorted bbox_idx the pointers stay inside [0, N]
    z = torch.zeros(4 + (P + 1 + 3) // 4 * 4 + max(N, 1), dtype=torch.int32, device=dev)
    seg = z[4:4 + P + 1]
    check(lib.yolat_segment_ptr(_i(bbox_idx, torch.int64, "bbox_idx"), N, P, seg.data_ptr(),
                                z[4 + (P + 1 + 3) // 4 * 4:].data_ptr(), z[0:1].data_ptr(), _stream()), "yolat_segment_ptr")
    return seg


def augment_batch(pos, x, seg_ptr, prop_ptr, bbox, params, cols=(3, 4)):
    """In place: the reference's random_transfer + update_bbox on a collated device batch (yolat_augment_batch).
    pos [N,2] / bbox [P,4] fp32 contiguous, x [N,C] fp32 (columns `cols` receive the positions), seg_ptr [P+1] int32,
    prop_ptr [B+1] int64, params [B,8] float64 (augment.AugParams.block()) — all on one device."""
    pos_ptr = _f(pos, "pos")
    N, P, B = int(pos.shape[0]), int(bbox.shape[0]), int(params.shape[0])
    if pos.dim() != 2 or pos.shape[1] != 2 or bbox.dim() != 2 or bbox.shape[1] != 4 or x.dim() != 2 or x.shape[0] != N:
        raise ValueError("augment_batch: pos must be [N,2], x [N,C], bbox [P,4]")
    if (N > 0 and not pos.is_contiguous()) or (P > 0 and not bbox.is_contiguous()):
        raise ValueError("augment_batch: pos and bbox must be contiguous")
    if not params.is_cuda or params.dtype != torch.float64 or params.dim() != 2 or params.shape[1] != 8 or \
            not params.is_contiguous():
        raise TypeError("augment_batch: params must be a contiguous [B,8] float64 CUDA tensor")
    if seg_ptr.shape[0] != P + 1 or prop_ptr.shape[0] != B + 1:
        raise ValueError("augment_batch: seg_ptr must be [P+1] and prop_ptr [B+1]")
    cx, cy = int(cols[0]), int(cols[1])
    if not (0 <= cx < x.shape[1] and 0 <= cy < x.shape[1]) or cx == cy:
        raise ValueError("augment_batch: position columns %r outside x [N,%d]" % (cols, x.shape[1]))
    for t in (x, seg_ptr, prop_ptr, bbox, params):
        if t.device != pos.device:
            raise RuntimeError("augment_batch: every operand must live on %s" % pos.device)
    check(lib.yolat_augment_batch(pos_ptr, _f(x, "x"), _ld(x), cx, cy, _i(seg_ptr, torch.int32, "seg_ptr"),
                                  _i(prop_ptr, torch.int64, "prop_ptr"), _f(bbox, "bbox"), params.data_ptr(), N, P, B,
                                  _stream()), "yolat_augment_batch")


# ---------------------------------------------------------------------------------------------
# dense
# ---------------------------------------------------------------------------------------------

def stats_buffer(M, C, device):
    return torch.empty(int(lib.yolat_bn_stats_elems(M, C)), dtype=torch.float32, device=device)


# YOLAT_STRICT_FP32=1: no bf16x6-emulated GEMM anywhere (csrc/x6.hpp; the C side reads the same variable)
STRICT_FP32 = os.environ.get("YOLAT_STRICT_FP32", "0") == "1"
X6_TRAIN_GEMM = not STRICT_FP32          # module flag (tests/test_gpu_ops.py flips it)
# the many-row training Linear on the bf16x6 rows kernel: measured EQUAL to the fp32-MFMA tiles (201 vs 199 us for
# [1.2 M, 64] -> [1.2 M, 64]: one 8-wave workgroup per CU, its load -> split -> MFMA -> store chain is not overlapped
# with a neighbour's), so it stays opt-in
X6_TRAIN_ROWS = False                    # module flag (tests/test_gpu_ops.py flips it)


def linear_fwd(A, W, bias, Y, a_pro=None, a_relu=False, o_pro=None, o_relu=False,
               accumulate=False, stats=None):
    """Y = epi(pro(A) @ W.T + bias).  a_pro / o_pro: (scale, shift) tensors or None."""
    M, K = A.shape
    Nout = W.shape[0]
    asc, ash = (a_pro if a_pro is not None else (None, None))
    osc, osh = (o_pro if o_pro is not None else (None, None))
    if _is_h(A) or _is_h(Y):
        if not (_is_h(A) and _is_h(Y)) or o_pro is not None or o_relu or accumulate:
            raise ValueError("bf16-storage linear_fwd: A and Y bfloat16, no output epilogue / accumulation")
        wwork = torch.empty(Nout * K, dtype=torch.bfloat16, device=A.device)
        check(lib.yolat_linear_fwd_h(_h(A, "A"), _ld(A), M, K, _f(asc, "a_scale", True), _f(ash, "a_shift", True),
                                     int(a_relu), _f(W, "W"), _ld(W), _f(bias, "bias", True), Nout, _h(Y, "Y"), _ld(Y),
                                     _f(stats, "stats", True), wwork.data_ptr(), _stream()), "yolat_linear_fwd_h")
        return Y
    if (X6_TRAIN_GEMM and stats is not None and a_pro is None and o_pro is None and not o_relu and not accumulate
            and bias is not None and M >= 1024 and K >= 256 and K % 16 == 0 and Nout >= 128 and _ld(A) % 4 == 0
            and A.data_ptr() % 16 == 0 and int(lib.yolat_gemm_x6_work_elems(M, Nout, K)) == 0):
        # many rows x long K in front of a training BatchNorm (the classifier's first layer at P = 8000): bf16x6-emulated
        # LDS-tiled GEMM with the statistics epilogue; the weight is packed per call
        packed = torch.empty(int(lib.yolat_gemm_x6_packed_elems(Nout, K)), dtype=torch.bfloat16, device=A.device)
        check(lib.yolat_gemm_x6_pack(_f(W, "W"), _ld(W), Nout, K, None, packed.data_ptr(), _stream()), "yolat_gemm_x6_pack")
        check(lib.yolat_gemm_x6_stats(_f(A, "A"), _ld(A), M, K, packed.data_ptr(), _f(bias, "bias"), Nout, _f(Y, "Y"), _ld(Y),
                                      _f(stats, "stats"), _stream()), "yolat_gemm_x6_stats")
        return Y
    if (X6_TRAIN_ROWS and o_pro is None and not o_relu and not accumulate and bias is not None and M >= 65536
            and K in (64, 128) and Nout % 64 == 0 and _ld(A) % 4 == 0 and A.data_ptr() % 16 == 0):
        # many rows x short K with a pre-activation output (the second edge Linear of a training conv layer, [E,64] ->
        # [E,64] + BatchNorm statistics): the bf16x6 rows kernel, A read once per 256 rows, weight split per call
        wsplit = torch.empty(3 * Nout * K, dtype=torch.bfloat16, device=A.device)
        check(lib.yolat_linear_fwd_rows_x6(_f(A, "A"), _ld(A), M, K, _f(asc, "a_scale", True), _f(ash, "a_shift", True),
                                           int(a_relu), _f(W, "W"), _ld(W), _f(bias, "bias"), Nout, _f(Y, "Y"), _ld(Y),
                                           _f(stats, "stats", True), wsplit.data_ptr(), _stream()),
              "yolat_linear_fwd_rows_x6")
        return Y
    check(lib.yolat_linear_fwd(_f(A, "A"), _ld(A), M, K, _f(asc, "a_scale", True), _f(ash, "a_shift", True),
                               int(a_relu), _f(W, "W"), _ld(W), _f(bias, "bias", True), Nout,
                               _f(osc, "o_scale", True), _f(osh, "o_shift", True), int(o_relu),
                               _f(Y, "Y"), _ld(Y), int(accumulate), _f(stats, "stats", True),
                               _stream()), "yolat_linear_fwd")
    return Y


def linear_sk_x6(A, W, bias, Y, o_pro=None, o_relu=False):
    """Y = epi(A @ W.T + bias) on the LDS-DMA split-K kernel with bf16x6-emulated products (csrc/linear_sk_x6.hip): few
    rows x long K, K % 128 == 0, 16-byte aligned rows.  Outside its shapes the library's error is raised."""
    M, K = A.shape
    Nout = W.shape[0]
    osc, osh = (o_pro if o_pro is not None else (None, None))
    check(lib.yolat_linear_sk_x6(_f(A, "A"), _ld(A), M, K, _f(W, "W"), _ld(W), _f(bias, "bias", True), Nout,
                                 _f(osc, "o_scale", True), _f(osh, "o_shift", True), int(o_relu), _f(Y, "Y"), _ld(Y),
                                 _stream()), "yolat_linear_sk_x6")
    return Y


def linear_fwd_wt(A, Wt, Y, accumulate=False):
    """Y = A @ Wt   (Wt: [K, Nout] row-major, e.g. dX = dY @ W)."""
    M, K = A.shape
    Nout = Wt.shape[1]
    if _is_h(A) or _is_h(Y):
        if not (_is_h(A) and _is_h(Y)) or accumulate:
            raise ValueError("bf16-storage linear_fwd_wt: A and Y bfloat16, no accumulation")
        wwork = torch.empty(Nout * K, dtype=torch.bfloat16, device=A.device)
        check(lib.yolat_linear_fwd_wt_h(_h(A, "A"), _ld(A), M, K, _f(Wt, "Wt"), _ld(Wt), Nout, _h(Y, "Y"), _ld(Y),
                                        wwork.data_ptr(), _stream()), "yolat_linear_fwd_wt_h")
        return Y
    if (X6_TRAIN_GEMM and not accumulate and M >= 1024 and K >= 256 and K % 16 == 0 and Nout >= 512
            and _ld(A) % 4 == 0 and A.data_ptr() % 16 == 0):
        # long-K, many-row backward GEMM (the classifier's first layer: dZ [P, 2304] = dC1 [P, 512] . Wc1): bf16x6-
        # emulated on the LDS-tiled kernel (gemm_x6.hip); the weight changes every step, so it is packed here (a few us)
        packed = torch.empty(int(lib.yolat_gemm_x6_packed_elems(Nout, K)), dtype=torch.bfloat16, device=A.device)
        check(lib.yolat_gemm_x6_pack_t(_f(Wt, "Wt"), _ld(Wt), Nout, K, packed.data_ptr(), _stream()),
              "yolat_gemm_x6_pack_t")
        work = torch.empty(max(1, int(lib.yolat_gemm_x6_work_elems(M, Nout, K))), dtype=torch.float32, device=A.device)
        check(lib.yolat_gemm_x6(_f(A, "A"), _ld(A), M, K, packed.data_ptr(), None, 0, Nout, _f(Y, "Y"), _ld(Y),
                                work.data_ptr(), _stream()), "yolat_gemm_x6")
        return Y
    check(lib.yolat_linear_fwd_wt(_f(A, "A"), _ld(A), M, K, _f(Wt, "Wt"), _ld(Wt), Nout, _f(Y, "Y"),
                                  _ld(Y), int(accumulate), _stream()), "yolat_linear_fwd_wt")
    return Y


# ---- "bf16_dense" training precision: the classifier / fusion_block_super GEMMs on bf16 operands (bf16_train.hip) ----
# every operand is rounded to nearest even inside the kernel, fp32 accumulation, no fall-back: a shape the kernels do not
# take raises ValueError

def _bt_aligned(t):
    """a weight view of the flat parameter buffer need not start on 16 bytes: the kernels read 16-byte pieces"""
    return t if t.data_ptr() % 16 == 0 else t.clone()


def _bt_check(rc, what, shape):
    if rc == -2:
        raise ValueError("bf16_dense training: %s does not take %s" % (what, shape))
    check(rc, what)


def bt_linear_fwd(A, W, bias, Y, a_pro=None, a_relu=False, stats=None):
    """Y = pro(A) @ W.T + bias on bf16 operands; stats: BatchNorm partials (stats_buffer(M, Nout))."""
    M, K = A.shape
    Nout = W.shape[0]
    asc, ash = (a_pro if a_pro is not None else (None, None))
    W = _bt_aligned(W)
    _bt_check(lib.yolat_bt_linear_fwd(_f(A, "A"), _ld(A), M, K, _f(asc, "a_scale", True), _f(ash, "a_shift", True),
                                      int(a_relu), _f(W, "W"), _ld(W), _f(bias, "bias", True), Nout, _f(Y, "Y"), _ld(Y),
                                      _f(stats, "stats", True), _stream()), "yolat_bt_linear_fwd",
              "[%d, %d] x [%d, %d]^T" % (M, K, Nout, K))
    return Y


def bt_linear_fwd_wt(A, Wt, Y, accumulate=False):
    """Y (+)= A @ Wt on bf16 operands (Wt: [K, Nout] row-major, e.g. dX = dY @ W)."""
    M, K = A.shape
    Nout = Wt.shape[1]
    Wt = _bt_aligned(Wt)
    _bt_check(lib.yolat_bt_linear_fwd_wt(_f(A, "A"), _ld(A), M, K, _f(Wt, "Wt"), _ld(Wt), Nout, _f(Y, "Y"), _ld(Y),
                                         int(accumulate), _stream()), "yolat_bt_linear_fwd_wt",
              "[%d, %d] x [%d, %d]" % (M, K, K, Nout))
    return Y


def bt_linear_bwd_w(dY, A, dW, db=None, a_pro=None, a_relu=False):
    """dW = dY.T @ pro(A) on bf16 operands; db = fp32 column sums of dY."""
    M, Nout = dY.shape
    K = A.shape[1]
    asc, ash = (a_pro if a_pro is not None else (None, None))
    work = torch.empty(int(lib.yolat_bt_linear_bwd_w_work_elems(M, Nout, K)), dtype=torch.float32, device=dY.device)
    _bt_check(lib.yolat_bt_linear_bwd_w(_f(dY, "dY"), _ld(dY), M, Nout, _f(A, "A"), _ld(A), K, _f(asc, "a_scale", True),
                                        _f(ash, "a_shift", True), int(a_relu), _f(dW, "dW"), _ld(dW), _f(db, "db", True),
                                        work.data_ptr(), _stream()), "yolat_bt_linear_bwd_w",
              "[%d, %d]^T x [%d, %d]" % (M, Nout, M, K))
    return dW


def linear_bwd_w(dY, A, dW, db=None, a_pro=None, a_relu=False, accumulate=False):
    M, Nout = dY.shape
    K = A.shape[1]
    asc, ash = (a_pro if a_pro is not None else (None, None))
    work = torch.empty(int(lib.yolat_linear_bwd_w_work_elems(M, Nout, K)), dtype=torch.float32,
                       device=dY.device)
    if _is_h(dY):
        check(lib.yolat_linear_bwd_w_h(_h(dY, "dY"), _ld(dY), M, Nout, _fh(A, "A"),
                                       int(_is_h(A)), _ld(A), K, _f(asc, "a_scale", True), _f(ash, "a_shift", True),
                                       int(a_relu), _f(dW, "dW"), _ld(dW), _f(db, "db", True), int(accumulate),
                                       work.data_ptr(), _stream()), "yolat_linear_bwd_w_h")
        return dW
    check(lib.yolat_linear_bwd_w(_f(dY, "dY"), _ld(dY), M, Nout, _f(A, "A"), _ld(A), K,
                                 _f(asc, "a_scale", True), _f(ash, "a_shift", True), int(a_relu),
                                 _f(dW, "dW"), _ld(dW), _f(db, "db", True), int(accumulate),
                                 work.data_ptr(), _stream()), "yolat_linear_bwd_w")
    return dW


class BnCsrGrad(object):
    """The gradient w.r.t. the input Y [E,C] of BatchNorm(train)+ReLU followed by the CSR mean aggregation, never
    materialised (bn_csr.hip): built from d_out [N,C] (gradient w.r.t. the aggregated output), the graph and the saved
    BatchNorm coefficients; `stats()` reduces dgamma / dbeta and the two coefficients the consumers need, then
    `bwd_w()` (dW = dY^T.pro(A), db) and `fwd_wt()` (dA = dY.W) form dY rows in their GEMM loaders."""

    def __init__(self, d_out, g, Y, save_mean, save_invstd, scale, shift, relu=True):
        from ._lib import BnCsrGrad as _S
        self.E, self.C, self.dev = Y.shape[0], Y.shape[1], Y.device
        self.coef = torch.empty(2 * self.C, dtype=torch.float32, device=self.dev)
        self._keep = (d_out, g, Y, save_mean, save_invstd, scale, shift, g.inv_deg())
        d = _S()
        d.d_out, d.ld_out = _f(d_out, "d_out"), _ld(d_out)
        d.dst, d.inv_deg = g.dst.data_ptr(), g.inv_deg().data_ptr()
        d.half = int(_is_h(Y))
        d.Y, d.ldy = _fh(Y, "Y"), _ld(Y)
        d.mean, d.invstd, d.scale, d.shift = _f(save_mean), _f(save_invstd), _f(scale), _f(shift)
        d.coef, d.relu = self.coef.data_ptr(), int(relu)
        self._d = d

    def stats(self, dgamma, dbeta, accumulate=False):
        work = torch.empty(int(lib.yolat_bn_csr_work_elems(self.E, self.C)), dtype=torch.float32, device=self.dev)
        check(lib.yolat_bn_csr_bwd_stats(ctypes.byref(self._d), self.E, self.C, _f(dgamma), _f(dbeta), int(accumulate),
                                         self.coef.data_ptr(), work.data_ptr(), _stream()), "yolat_bn_csr_bwd_stats")
        return self

    def bwd_w(self, A, dW, db=None, a_pro=None, a_relu=False, accumulate=False):
        K = A.shape[1]
        asc, ash = (a_pro if a_pro is not None else (None, None))
        work = torch.empty(int(lib.yolat_linear_bwd_w_work_elems(self.E, self.C, K)), dtype=torch.float32, device=self.dev)
        check(lib.yolat_linear_bwd_w_csr(ctypes.byref(self._d), self.E, self.C, _f(A, "A"), _ld(A), K,
                                         _f(asc, "a_scale", True), _f(ash, "a_shift", True), int(a_relu), _f(dW, "dW"),
                                         _ld(dW), _f(db, "db", True), int(accumulate), work.data_ptr(), _stream()),
              "yolat_linear_bwd_w_csr")
        return dW

    def bwd_w_and_x(self, A, W, dW, db, dA, a_pro=None, a_relu=False, accumulate=False, next_bn=None):
        """dW (+)= dY^T . pro(A), db (+)= column sums, dA = dY . W in one kernel (C = K = 64).  next_bn = (save_mean,
        save_invstd, dgamma, dbeta) of the BatchNorm behind a_pro: its backward statistics on dA come out of the same
        kernel; returns their coefficient vector [2C] for bn_relu_bwd_apply (else None)."""
        asc, ash = (a_pro if a_pro is not None else (None, None))
        work = torch.empty(int(lib.yolat_bn_csr_l2_bwd_work_elems()), dtype=torch.float32, device=self.dev)
        hp = bool(self._d.half)
        if _is_h(A) != hp or _is_h(dA) != hp:
            raise ValueError("BnCsrGrad.bwd_w_and_x: A and dA must use the storage type of Y")
        coef1 = None
        nm = ni = ng = nb = nc = None
        if next_bn is not None:
            coef1 = torch.empty(2 * self.C, dtype=torch.float32, device=self.dev)
            nm, ni, ng, nb, nc = _f(next_bn[0]), _f(next_bn[1]), _f(next_bn[2]), _f(next_bn[3]), coef1.data_ptr()
        check(lib.yolat_bn_csr_l2_bwd(ctypes.byref(self._d), self.E, _fh(A, "A", hp), _ld(A),
                                      _f(asc, "a_scale", True), _f(ash, "a_shift", True), int(a_relu), _f(W, "W"), _ld(W),
                                      _f(dW, "dW"), _ld(dW), _f(db, "db", True), int(accumulate),
                                      _fh(dA, "dA", hp), _ld(dA), work.data_ptr(), nm, ni, ng, nb, nc,
                                      _stream()), "yolat_bn_csr_l2_bwd")
        return coef1

    def fwd_wt(self, W, dA):
        check(lib.yolat_linear_fwd_wt_csr(ctypes.byref(self._d), self.E, self.C, _f(W, "W"), _ld(W), W.shape[1],
                                          _f(dA, "dA"), _ld(dA), _stream()), "yolat_linear_fwd_wt_csr")
        return dA


def bn_relu_bwd_apply(dZ, Y, save_mean, save_invstd, scale, shift, relu, coef, dY):
    """The apply pass of bn_relu_bwd alone, with the coefficient vector [2C] = (c1 | c2) given."""
    M, C = Y.shape
    hp = _is_h(Y)
    check(lib.yolat_bn_relu_bwd_apply(_fh(dZ, "dZ", hp), _ld(dZ), _fh(Y, "Y"), _ld(Y),
                                      M, C, _f(save_mean), _f(save_invstd), _f(scale), _f(shift), int(relu), _f(coef),
                                      _fh(dY, "dY", hp), _ld(dY), int(hp), _stream()),
          "yolat_bn_relu_bwd_apply")
    return dY


def bn_finalize(stats, M, bn, scale, shift, save_mean, save_invstd, update_running=True):
    C = bn.num_features
    rm = bn.running_mean if (update_running and bn.track_running_stats) else None
    rv = bn.running_var if (update_running and bn.track_running_stats) else None
    mom = 0.1 if bn.momentum is None else float(bn.momentum)
    if rm is not None:
        bump_weight_epoch()
    check(lib.yolat_bn_finalize(_f(stats), M, C, _f(bn.weight), _f(bn.bias), _f(rm, "rm", True),
                                _f(rv, "rv", True), mom, float(bn.eps), _f(save_mean),
                                _f(save_invstd), _f(scale), _f(shift), _stream()), "yolat_bn_finalize")


def bn_eval_coeffs(bn, scale, shift):
    check(lib.yolat_bn_eval_coeffs(_f(bn.weight), _f(bn.bias), _f(bn.running_mean), _f(bn.running_var),
                                   float(bn.eps), bn.num_features, _f(scale), _f(shift), _stream()),
          "yolat_bn_eval_coeffs")


def scale_shift_relu(Y, scale, shift, relu, Z):
    M, C = Y.shape
    check(lib.yolat_scale_shift_relu(_f(Y), _ld(Y), M, C, _f(scale, "scale", True), _f(shift, "shift", True),
                                     int(relu), _f(Z), _ld(Z), _stream()), "yolat_scale_shift_relu")
    return Z


def bn_relu_bwd(dZ, Y, gamma, save_mean, save_invstd, scale, shift, relu, dgamma, dbeta, dY,
                accumulate=False):
    M, C = Y.shape
    work = torch.empty(int(lib.yolat_bn_bwd_work_elems(M, C)), dtype=torch.float32, device=Y.device)
    if _is_h(Y):
        check(lib.yolat_bn_relu_bwd_h(_h(dZ, "dZ"), _ld(dZ), _h(Y, "Y"), _ld(Y), M, C, _f(save_mean), _f(save_invstd),
                                      _f(scale), _f(shift), int(relu), _f(dgamma), _f(dbeta), int(accumulate),
                                      _h(dY, "dY"), _ld(dY), work.data_ptr(), _stream()), "yolat_bn_relu_bwd_h")
        return dY
    check(lib.yolat_bn_relu_bwd(_f(dZ), _ld(dZ), _f(Y), _ld(Y), M, C, _f(gamma), _f(save_mean),
                                _f(save_invstd), _f(scale), _f(shift), int(relu), _f(dgamma),
                                _f(dbeta), int(accumulate), _f(dY), _ld(dY), work.data_ptr(),
                                _stream()), "yolat_bn_relu_bwd")
    return dY


# ---------------------------------------------------------------------------------------------
# leaky activations (csrc/act.hip): act(y) = y > 0 ? y : a * y, the slope a read from device memory
# ---------------------------------------------------------------------------------------------

ACT_RELU, ACT_LEAKYRELU, ACT_PRELU = 0, 1, 2


def act_kind(mod):
    """YOLAT_ACT_* of an activation module (torch_nn.py:9-20)."""
    if isinstance(mod, torch.nn.PReLU):
        return ACT_PRELU
    if isinstance(mod, torch.nn.LeakyReLU):
        return ACT_LEAKYRELU
    if isinstance(mod, torch.nn.ReLU):
        return ACT_RELU
    raise NotImplementedError("act layer %s has no MI355X kernel" % mod.__class__.__name__)


def act_slope(mod, dev):
    """The one-float device tensor a kernel reads the slope of `mod` from: a PReLU's weight itself (in-place edits and
    Adam steps are seen by the next launch), for a LeakyReLU a constant cached on the module per device."""
    if isinstance(mod, torch.nn.PReLU):
        w = mod.weight
        if w.numel() != 1:
            raise ValueError("act prelu: num_parameters must be 1 (the reference's n_prelu), got %d" % w.numel())
        if not w.is_cuda or w.dtype != torch.float32:
            raise RuntimeError("act prelu: the slope must be a float32 CUDA (ROCm) tensor")
        return w
    cache = mod.__dict__.setdefault("_yolat_slope", {})
    t = cache.get(dev)
    if t is None or float(mod.negative_slope) != cache.get("value"):
        cache.clear()
        t = cache[dev] = torch.full((1,), float(mod.negative_slope), dtype=torch.float32, device=dev)
        cache["value"] = float(mod.negative_slope)
    return t


def scale_shift_act(Y, scale, shift, slope, Z):
    """Z = act(Y * scale + shift) (scale None: act(Y)); Z may be Y."""
    M, C = Y.shape
    check(lib.yolat_scale_shift_act(_f(Y), _ld(Y), M, C, _f(scale, "scale", True), _f(shift, "shift", True),
                                    _f(slope, "slope"), _f(Z), _ld(Z), _stream()), "yolat_scale_shift_act")
    return Z


def segment_act_max(Y, slope, g, out):
    """out[p] = max over the rows of proposal p of act(Y[r]) (0 for an empty proposal): signed values, no atomics."""
    check(lib.yolat_segment_act_max(_f(Y), _ld(Y), Y.shape[0], Y.shape[1], _f(slope, "slope"), g.seg_ptr.data_ptr(), g.P, _f(out),
                                    _ld(out), _stream()), "yolat_segment_act_max")
    return out


def bn_act_bwd(dZ, Y, save_mean, save_invstd, scale, shift, slope, dgamma, dbeta, dslope, dY, accumulate=False):
    """Backward of act(BN_train(Y)): bn_relu_bwd with the slope, and dslope (None for a LeakyReLU) = sum_{y' <= 0} dZ * y'."""
    M, C = Y.shape
    work = torch.empty(int(lib.yolat_bn_act_bwd_work_elems(M, C)), dtype=torch.float32, device=Y.device)
    check(lib.yolat_bn_act_bwd(_f(dZ), _ld(dZ), _f(Y), _ld(Y), M, C, _f(save_mean), _f(save_invstd), _f(scale), _f(shift),
                               _f(slope, "slope"), _f(dgamma), _f(dbeta), _f(dslope, "dslope", True), int(accumulate),
                               _f(dY), _ld(dY), work.data_ptr(), _stream()), "yolat_bn_act_bwd")
    return dY


def fusion_pair_eval_act(A, lin_f, fold_f, slope_f, g, pool, S=None, lin_s=None, fold_s=None, slope_s=None, Ys=None):
    """yolat_fusion_pair_eval_act: pool[P,F] = per-proposal max of act(bn(lin_f(A))), Ys = act(bn(lin_s(S))); fold_* = the
    eval BatchNorm as (scale, shift)."""
    N, D = A.shape
    F = lin_f.weight.shape[0]
    work = torch.empty(int(lib.yolat_fusion_pair_eval_act_work_elems(N, F)), dtype=torch.float32, device=A.device)
    has_s = S is not None
    check(lib.yolat_fusion_pair_eval_act(
        _f(A), _ld(A), N, D, _f(lin_f.weight), _f(lin_f.bias, "bias", True), _f(fold_f[0]), _f(fold_f[1]), F, _f(slope_f),
        g.seg_ptr.data_ptr(), _f(pool), _ld(pool), _f(S, "S", True), _ld(S) if has_s else 0, g.P,
        _f(lin_s.weight) if has_s else None, _f(lin_s.bias, "bias", True) if has_s else None,
        _f(fold_s[0]) if has_s else None, _f(fold_s[1]) if has_s else None, _f(slope_s) if has_s else None,
        _f(Ys, "Ys", True), _ld(Ys) if has_s else 0, work.data_ptr(), _stream()), "yolat_fusion_pair_eval_act")
    return pool


# ---------------------------------------------------------------------------------------------
# row norms (csrc/rownorm.hip): nn.LayerNorm / nn.InstanceNorm1d(affine=False) on [M, nc] — one per-row arithmetic
# ---------------------------------------------------------------------------------------------

NORM_BATCH, NORM_LAYER, NORM_INSTANCE = 0, 1, 2
RN_ROWS = 128          # YOLAT_RN_ROWS: rows per workgroup of the fused eval kernel
RN_ROUTE_AUTO, RN_ROUTE_FUSED, RN_ROUTE_MATERIALISE = 0, 1, 2       # YOLAT_RN_ROUTE_*
RN_ROUTE_BF16 = 0x100  # YOLAT_RN_ROUTE_BF16: or-ed into rn_route, the opt-in of a row-norm base for the bf16-storage forward


def is_rownorm(mod):
    return isinstance(mod, (torch.nn.LayerNorm, torch.nn.InstanceNorm1d))


def norm_kind(mod):
    """YOLAT_NORM_* of a norm module (torch_nn.py:23-34)."""
    if isinstance(mod, torch.nn.BatchNorm1d):
        return NORM_BATCH
    if isinstance(mod, torch.nn.LayerNorm):
        if len(mod.normalized_shape) != 1 or mod.weight is None or mod.bias is None:
            raise NotImplementedError("norm layer: LayerNorm over one dimension with weight and bias (the reference's)")
        return NORM_LAYER
    if isinstance(mod, torch.nn.InstanceNorm1d):
        if mod.affine or mod.track_running_stats:
            raise NotImplementedError("norm instance: InstanceNorm1d(affine=False, track_running_stats=False) (the reference's)")
        return NORM_INSTANCE
    raise NotImplementedError("norm layer %s has no MI355X kernel" % mod.__class__.__name__)


def rownorm_params(mod):
    """(gamma, beta, eps) of a row-norm module; gamma / beta None for the instance norm."""
    if norm_kind(mod) == NORM_LAYER:
        return mod.weight, mod.bias, float(mod.eps)
    return None, None, float(mod.eps)


def rownorm_act(Y, gamma, beta, eps, relu, Z, save_mean=None, save_rstd=None):
    """Z = relu?(rownorm(Y) * gamma + beta); Z may be Y; save_mean / save_rstd [M] optional."""
    M, C = Y.shape
    check(lib.yolat_rownorm_act(_f(Y), _ld(Y), M, C, _f(gamma, "gamma", True), _f(beta, "beta", True), float(eps), int(bool(relu)),
                                _f(Z), _ld(Z), _f(save_mean, "save_mean", True), _f(save_rstd, "save_rstd", True), _stream()),
          "yolat_rownorm_act")
    return Z


def rownorm_act_bwd(dZ, Y, save_mean, save_rstd, gamma, beta, relu, dgamma, dbeta, dY, accumulate=False):
    """Backward of rownorm_act from the saved pre-norm Y, mean and rstd; dgamma / dbeta None with gamma None."""
    M, C = Y.shape
    work = None
    if gamma is not None:
        work = torch.empty(int(lib.yolat_rownorm_act_bwd_work_elems(M, C)), dtype=torch.float32, device=Y.device)
    check(lib.yolat_rownorm_act_bwd(_f(dZ), _ld(dZ), _f(Y), _ld(Y), M, C, _f(save_mean), _f(save_rstd), _f(gamma, "gamma", True),
                                    _f(beta, "beta", True), int(bool(relu)), _f(dgamma, "dgamma", True), _f(dbeta, "dbeta", True),
                                    int(accumulate), _f(dY), _ld(dY), work.data_ptr() if work is not None else None,
                                    _stream()), "yolat_rownorm_act_bwd")
    return dY


def rownorm_center(weight, bias):
    """The operands of yolat_fusion_pair_eval_x6_rn from a Linear [F, D]: Wc = W - mean over the F outputs, bc = b - mean(b)
    (taken in float64, rounded once), so that A . Wc^T + bc is the product with its row mean already removed."""
    w = weight.detach().double()
    wc = (w - w.mean(0, keepdim=True)).float().contiguous()
    b = bias.detach().double() if bias is not None else torch.zeros(weight.shape[0], dtype=torch.float64, device=weight.device)
    return wc, (b - b.mean()).float().contiguous()


def split_bf16x3(w, row_scale=None):
    """Exact 3-way bfloat16 split (hi, mid, lo) of a contiguous fp32 matrix, rows scaled first when row_scale is given
    (yolat_split_bf16x3) — the one caller of that entry point (plan.py's weight splits come here too)."""
    rows, cols = w.shape
    parts = [torch.empty(rows * cols, dtype=torch.bfloat16, device=w.device) for _ in range(3)]
    check(lib.yolat_split_bf16x3(_f(w), cols, rows, cols, _f(row_scale, "row_scale", True), parts[0].data_ptr(), parts[1].data_ptr(), parts[2].data_ptr(),
                                 _stream()), "yolat_split_bf16x3")
    return parts


def split_f16x2(w, row_scale=None):
    """Scaled two-term half-precision split (hi [rows, cols], lo [rows, cols], scale exponent per row [rows] int32) of a
    contiguous fp32 matrix, rows scaled first when row_scale is given (yolat_split_f16x2, csrc/f16x3.hpp)."""
    rows, cols = w.shape
    hi, lo = (torch.empty(rows, cols, dtype=torch.float16, device=w.device) for _ in range(2))
    exps = torch.empty(rows, dtype=torch.int32, device=w.device)
    check(lib.yolat_split_f16x2(_f(w), cols, rows, cols, _f(row_scale, "row_scale", True), hi.data_ptr(), lo.data_ptr(),
                                exps.data_ptr(), _stream()), "yolat_split_f16x2")
    return hi, lo, exps


def fusion_pair_eval_x6_rn(A, lin_f, gb_f, node_seg, pool, S, lin_s, gb_s, Ys, eps):
    """yolat_fusion_pair_eval_x6_rn: pool[P,F] (zero-filled by the caller) = per-proposal max of relu(rownorm(lin_f(A)) g + b),
    Ys = the same of lin_s(S) stored; gb_* = (gamma, beta) or (None, None)."""
    N, D = A.shape
    F = lin_f.weight.shape[0]
    wf, tf = rownorm_center(lin_f.weight, lin_f.bias)
    ws, ts = rownorm_center(lin_s.weight, lin_s.bias)
    pf, ps = split_bf16x3(wf), split_bf16x3(ws)
    check(lib.yolat_fusion_pair_eval_x6_rn(
        _f(A), _ld(A), N, D, pf[0].data_ptr(), pf[1].data_ptr(), pf[2].data_ptr(), _f(tf), F, _f(gb_f[0], "gamma", True),
        _f(gb_f[1], "beta", True), node_seg.data_ptr(), _f(pool), _ld(pool), _f(S), _ld(S), S.shape[0], ps[0].data_ptr(),
        ps[1].data_ptr(), ps[2].data_ptr(), _f(ts), _f(gb_s[0], "gamma", True), _f(gb_s[1], "beta", True), _f(Ys), _ld(Ys),
        float(eps), _stream()), "yolat_fusion_pair_eval_x6_rn")
    return pool


def fusion_pair_eval_rn(A, lin_f, gb_f, node_seg, pool, S, lin_s, gb_s, Ys, eps):
    """yolat_fusion_pair_eval_rn: the materialising form of fusion_pair_eval_x6_rn, any D / F."""
    N, D = A.shape
    F = lin_f.weight.shape[0]
    work = torch.empty(int(lib.yolat_fusion_pair_eval_rn_work_elems(N, F)), dtype=torch.float32, device=A.device)
    check(lib.yolat_fusion_pair_eval_rn(
        _f(A), _ld(A), N, D, _f(lin_f.weight), _f(lin_f.bias, "bias", True), F, _f(gb_f[0], "gamma", True),
        _f(gb_f[1], "beta", True), node_seg.data_ptr(), _f(pool), _ld(pool), _f(S), _ld(S), S.shape[0], _f(lin_s.weight),
        _f(lin_s.bias, "bias", True), _f(gb_s[0], "gamma", True), _f(gb_s[1], "beta", True), _f(Ys), _ld(Ys), float(eps),
        work.data_ptr(), _stream()), "yolat_fusion_pair_eval_rn")
    return pool


# ---------------------------------------------------------------------------------------------
# edge convolution
# ---------------------------------------------------------------------------------------------

def edge_lin1_fwd(x, g, W1, b1, H1, o_pro=None, o_relu=False, stats=None):
    N, Cin = x.shape
    C = W1.shape[0]
    osc, osh = (o_pro if o_pro is not None else (None, None))
    check(lib.yolat_edge_lin1_fwd(_f(x, "x"), _ld(x), N, Cin, g.src.data_ptr(), g.dst.data_ptr(),
                                  g.attr.data_ptr(), g.E, _f(W1), _ld(W1), _f(b1, "b1", True), C,
                                  _f(osc, "o_scale", True), _f(osh, "o_shift", True), int(o_relu),
                                  _f(H1), _ld(H1), _f(stats, "stats", True), _stream()),
          "yolat_edge_lin1_fwd")
    return H1


def split_w1(W1, Cin):
    """yolat_conv_split_w1: Wuv [2C,Cin] = [W1a - W1b | W1b] (rows), Wc4 [C,4] = the attr columns."""
    C = W1.shape[0]
    if not W1.is_contiguous():
        raise ValueError("W1 must be contiguous")
    wuv = torch.empty(2 * C, Cin, dtype=torch.float32, device=W1.device)
    wc4 = torch.empty(C, 4, dtype=torch.float32, device=W1.device)
    check(lib.yolat_conv_split_w1(_f(W1), Cin, C, wuv.data_ptr(), wc4.data_ptr(), _stream()), "yolat_conv_split_w1")
    return wuv, wc4


def attr_dw(dH1, g, dwc4, db1=None):
    """dWc4 [C, 4] = dH1^T . attr, db1 = column sums of dH1: the streaming reduction yolat_edge_attr_dw (C = 64, rows
    16-byte aligned); other shapes fall back to the general weight-gradient GEMM."""
    E, C = dH1.shape
    half = _is_h(dH1)
    if C == 64 and dH1.stride(1) == 1 and dH1.stride(0) % 4 == 0 and dH1.data_ptr() % 16 == 0 and E > 0:
        work = torch.empty(int(lib.yolat_edge_attr_dw_work_elems(E)), dtype=torch.float32, device=dH1.device)
        check(lib.yolat_edge_attr_dw(dH1.data_ptr(), dH1.stride(0), 1 if half else 0, g.attr.data_ptr(), E, C, _f(dwc4),
                                     _f(db1, "db1", True), work.data_ptr(), _stream()), "yolat_edge_attr_dw")
        return dwc4
    return linear_bwd_w(dH1, g.attr, dwc4, db1)


def bn_apply_edge_sums(dA1, H1, save_mean, save_invstd, scale, shift, relu, coef, g, db1):
    """The BatchNorm + ReLU backward apply pass in front of the factorised first edge Linear, fused with the consumers
    that read its result in CSR order (yolat_bn_apply_edge_sums): dA1 -> dH1 in place, returns (dUV [N, 128] with the dU
    half written, dWc4 [64, 4]); db1 is written.  Hand both to edge_lin1_bwd_factorised(..., partial=(dUV, dWc4))."""
    E, C = H1.shape
    N = g.N
    hp = _is_h(H1)
    dUV = torch.empty(N, 2 * C, dtype=torch.float32, device=H1.device)
    dwc4 = torch.empty(C, 4, dtype=torch.float32, device=H1.device)
    work = torch.empty(int(lib.yolat_bn_apply_edge_sums_work_elems(N)), dtype=torch.float32, device=H1.device)
    check(lib.yolat_bn_apply_edge_sums(_fh(dA1, "dA1", hp), _ld(dA1), _fh(H1, "H1"), _ld(H1), dA1.data_ptr(), _ld(dA1),
                                       int(hp), E, _f(save_mean), _f(save_invstd),
                                       _f(scale), _f(shift), int(relu), _f(coef), g.row_ptr.data_ptr(), g.attr.data_ptr(), N,
                                       dUV.data_ptr(), 2 * C, dwc4.data_ptr(), _f(db1, "db1", True), work.data_ptr(),
                                       _stream()), "yolat_bn_apply_edge_sums")
    return dUV, dwc4


def edge_lin1_bwd_factorised(dH1, x, g, W1, dW1, db1, dx=None, dx_accumulate=False, wuv=None, side=None, partial=None):
    """Backward of the first edge Linear through the per-node products (see yolat_edge_uv_sums): writes dW1, db1 and,
    when `dx` is given, (accumulates) the gradient w.r.t. the node features.  C = 64; pays when E >> N.
    partial = (dUV, dWc4) from bn_apply_edge_sums: the dU half, dWc4 and db1 exist already — only the gathered dV half
    is left to sum."""
    N, Cin = x.shape
    C = W1.shape[0]
    g.ensure_csc()
    if wuv is None:
        wuv, _ = split_w1(W1, Cin)
    dwc4_done = None
    if partial is not None:
        dUV, dwc4_done = partial
        check(lib.yolat_edge_uv_sums_v(dH1.data_ptr(), _ld(dH1), int(_is_h(dH1)), g.col_ptr.data_ptr(), g.slots.data_ptr(),
                                       N, C, dUV.data_ptr(), 2 * C, _stream()), "yolat_edge_uv_sums_v")
    else:
        dUV = torch.empty(N, 2 * C, dtype=torch.float32, device=x.device)
        fn = lib.yolat_edge_uv_sums_h if _is_h(dH1) else lib.yolat_edge_uv_sums
        check(fn(_fh(dH1), _ld(dH1), g.row_ptr.data_ptr(), g.col_ptr.data_ptr(), g.slots.data_ptr(), N, C,
                 dUV.data_ptr(), 2 * C, _stream()), fn.__name__)
    def weight_grads():
        dwuv = torch.empty(2 * C, Cin, dtype=torch.float32, device=x.device)
        linear_bwd_w(dUV, x, dwuv)
        if dwc4_done is not None:
            dwc4 = dwc4_done
        else:
            dwc4 = torch.empty(C, 4, dtype=torch.float32, device=x.device)
            attr_dw(dH1, g, dwc4, db1)
        check(lib.yolat_conv_merge_dw1(dwuv.data_ptr(), dwc4.data_ptr(), Cin, C, _f(dW1), _ld(dW1), 0, _stream()),
              "yolat_conv_merge_dw1")
    # `side` (engine._on_side): the three weight-gradient launches on a second stream, beside the dx GEMM below and
    # whatever the caller issues next — nothing in the backward reads dW1 / db1
    if side is not None:
        side(weight_grads, (dUV, x, dH1, g.attr, dwc4_done))
    else:
        weight_grads()
    if dx is not None:
        linear_fwd_wt(dUV, wuv, dx, accumulate=dx_accumulate)
    return dW1


def edge_lin1_fwd_factorised(x, g, W1, b1, H1, stats=None, keep=None):
    """Same result as edge_lin1_fwd (to fp32 rounding) through the per-node products: UV = x.[W1a-W1b | W1b]^T by a
    dense GEMM over the N nodes, then a gather-add over the E edges (csrc/edge_ops.hip, yolat_edge_uv_lin1_fwd).  Pays
    when E >> N; Cin == C == 64 only."""
    N, Cin = x.shape
    C = W1.shape[0]
    wuv, wc4 = split_w1(W1, Cin)
    if keep is not None:
        keep["wuv"] = wuv               # the backward of the same step needs the same split (edge_lin1_bwd_factorised)
    uv = torch.empty(N, 2 * C, dtype=torch.float32, device=x.device)
    linear_fwd(x, wuv, None, uv)
    fn = lib.yolat_edge_uv_lin1_fwd_h if _is_h(H1) else lib.yolat_edge_uv_lin1_fwd
    check(fn(uv.data_ptr(), 2 * C, g.src.data_ptr(), g.dst.data_ptr(), g.attr.data_ptr(), g.E, wc4.data_ptr(),
             _f(b1, "b1", True), C, _fh(H1, "H1"), _ld(H1), _f(stats, "stats", True), _stream()), fn.__name__)
    return H1


def fold_factorised_layer(wuv, wc4, b1, s1, t1, b2, s2, t2):
    """Folded form of a factorised eval conv layer (include/yolat_hip.h, yolat_conv_eval.{Wuvf, uvb, Wc4f, t2f}):
    nn.1's folded BatchNorm (s1, t1) and the bias b1 move into the per-node products and the attr weights, b2 into the
    shift of nn.4, so the per-edge arithmetic is  h1 = relu(U'[dst] + V'[src] + Wc4f.attr),
    message = relu(s2 * (W2.h1) + t2f).  Elementwise work on [C]- / weight-sized tensors, once per weight version."""
    zeros = torch.zeros_like(s1)
    b1 = zeros if b1 is None else b1.detach()
    b2 = zeros if b2 is None else b2.detach()
    wuvf = (wuv * torch.cat([s1, s1]).unsqueeze(1)).contiguous()
    uvb = torch.cat([s1 * b1 + t1, zeros]).contiguous()
    wc4f = (wc4 * s1.unsqueeze(1)).contiguous()
    t2f = (s2 * b2 + t2).contiguous()
    return wuvf, uvb, wc4f, t2f


EDGE_AUTO, EDGE_TILES, EDGE_WS_F32, EDGE_WS_X6 = 0, 1, 2, 3


def edge_uv_mlp2_mean_eval(UV, g, wc4, b1, pro1, W2, b2, pro2, f_out, variant=EDGE_AUTO):
    """f_out[n] += mean over the CSR row of n of relu(s2*(W2.relu(s1*(U[dst]+V[src]+wc4.attr+b1)+t1)+b2)+t2)
    (yolat_edge_uv_mlp2_mean_eval_variant; b1 / pro1 / b2 may be None)."""
    s1, t1 = pro1 if pro1 is not None else (None, None)
    s2, t2 = pro2 if pro2 is not None else (None, None)
    check(lib.yolat_edge_uv_mlp2_mean_eval_variant(_f(UV, "UV"), _ld(UV), g.src.data_ptr(), g.dst.data_ptr(),
                                                   g.attr.data_ptr(), g.row_ptr.data_ptr(), g.N, g.E, _f(wc4),
                                                   _f(b1, "b1", True), _f(s1, "s1", True), _f(t1, "t1", True), _f(W2),
                                                   _f(b2, "b2", True), _f(s2, "s2", True), _f(t2, "t2", True),
                                                   W2.shape[0], _f(f_out), _ld(f_out), int(variant), _stream()),
          "yolat_edge_uv_mlp2_mean_eval_variant")
    return f_out


def edge_uv_mlp2_mean_eval_mt(UV, g, wc4, b1, pro1, W2, b2, pro2, f_out, tiles_per_wg=1):
    """edge_uv_mlp2_mean_eval on the node-tile kernel with `tiles_per_wg` consecutive tiles per workgroup
    (yolat_edge_uv_mlp2_mean_eval_mt; 1 = the one-tile kernel; bit-identical f_out at every value)."""
    s1, t1 = pro1 if pro1 is not None else (None, None)
    s2, t2 = pro2 if pro2 is not None else (None, None)
    check(lib.yolat_edge_uv_mlp2_mean_eval_mt(_f(UV, "UV"), _ld(UV), g.src.data_ptr(), g.dst.data_ptr(),
                                              g.attr.data_ptr(), g.row_ptr.data_ptr(), g.N, g.E, _f(wc4),
                                              _f(b1, "b1", True), _f(s1, "s1", True), _f(t1, "t1", True), _f(W2),
                                              _f(b2, "b2", True), _f(s2, "s2", True), _f(t2, "t2", True),
                                              W2.shape[0], _f(f_out), _ld(f_out), int(tiles_per_wg), _stream()),
          "yolat_edge_uv_mlp2_mean_eval_mt")
    return f_out


def edge_mlp2_eval(x, g, W1, b1, pro1, W2, b2, pro2, H2):
    """Eval-mode two-layer edge MLP in one kernel (BN folded into pro1/pro2 = (scale, shift))."""
    N, Cin = x.shape
    C = W1.shape[0]
    if not (W1.is_contiguous() and W2.is_contiguous()):
        raise ValueError("W1 / W2 must be contiguous")
    check(lib.yolat_edge_mlp2_eval(_f(x, "x"), _ld(x), N, Cin, g.src.data_ptr(), g.dst.data_ptr(), g.attr.data_ptr(),
                                   g.E, _f(W1), _f(b1), _f(pro1[0]), _f(pro1[1]), _f(W2), _f(b2), _f(pro2[0]),
                                   _f(pro2[1]), C, _f(H2), _ld(H2), _stream()), "yolat_edge_mlp2_eval")
    return H2


def edge_lin1_bwd_w(dH1, x, g, dW1, db1=None, accumulate=False):
    E, C = dH1.shape[0], dW1.shape[0]
    N, Cin = x.shape
    work = torch.empty(int(lib.yolat_linear_bwd_w_work_elems(g.E, C, 2 * Cin + 4)), dtype=torch.float32,
                       device=x.device)
    check(lib.yolat_edge_lin1_bwd_w(_f(dH1), _ld(dH1), g.E, C, _f(x), _ld(x), N, Cin, g.src.data_ptr(),
                                    g.dst.data_ptr(), g.attr.data_ptr(), _f(dW1), _ld(dW1),
                                    _f(db1, "db1", True), int(accumulate), work.data_ptr(), _stream()),
          "yolat_edge_lin1_bwd_w")
    return dW1


def edge_lin1_bwd_x(dH1, W1, Cin, dG):
    C = W1.shape[0]
    check(lib.yolat_edge_lin1_bwd_x(_f(dH1), _ld(dH1), dH1.shape[0], C, _f(W1), _ld(W1), Cin, _f(dG),
                                    _ld(dG), _stream()), "yolat_edge_lin1_bwd_x")
    return dG


def edge_scatter_bwd(dG, Cin, g, dX, accumulate=False):
    g.ensure_csc()
    check(lib.yolat_edge_scatter_bwd(_f(dG), _ld(dG), Cin, g.row_ptr.data_ptr(), g.col_ptr.data_ptr(),
                                     g.slots.data_ptr(), g.N, _f(dX), _ld(dX), int(accumulate),
                                     _stream()), "yolat_edge_scatter_bwd")
    return dX


def csr_mean_fwd(H, g, out, h_pro=None, h_relu=False, accumulate=False):
    C = out.shape[1]
    hs, hb = (h_pro if h_pro is not None else (None, None))
    if _is_h(H):
        check(lib.yolat_csr_mean_fwd_h(_h(H, "H"), _ld(H), C, _f(hs, "h_scale", True), _f(hb, "h_shift", True),
                                       int(h_relu), g.row_ptr.data_ptr(), g.N, _f(out), _ld(out), int(accumulate),
                                       _stream()), "yolat_csr_mean_fwd_h")
        return out
    check(lib.yolat_csr_mean_fwd(_f(H, "H", g.E == 0), _ld(H) if H is not None else C, C,
                                 _f(hs, "h_scale", True), _f(hb, "h_shift", True), int(h_relu),
                                 g.row_ptr.data_ptr(), g.N, _f(out), _ld(out), int(accumulate),
                                 _stream()), "yolat_csr_mean_fwd")
    return out


def csr_mean_bwd(dOut, g, dM):
    C = dOut.shape[1]
    fn = lib.yolat_csr_mean_bwd_h if _is_h(dM) else lib.yolat_csr_mean_bwd
    check(fn(_f(dOut), _ld(dOut), C, g.row_ptr.data_ptr(), g.dst.data_ptr(), g.E, _fh(dM, "dM"), _ld(dM), _stream()),
          fn.__name__)
    return dM


# ---------------------------------------------------------------------------------------------
# proposal pooling
# ---------------------------------------------------------------------------------------------

def segment_mean_fwd(X, g, Y, x_pro=None, x_relu=False):
    D = X.shape[1]
    xs, xb = (x_pro if x_pro is not None else (None, None))
    check(lib.yolat_segment_mean_fwd(_f(X), _ld(X), D, _f(xs, "x_scale", True), _f(xb, "x_shift", True),
                                     int(x_relu), g.seg_ptr.data_ptr(), g.P, _f(Y), _ld(Y), _stream()),
          "yolat_segment_mean_fwd")
    return Y


def segment_max_fwd(X, g, Y, arg=None, x_pro=None, x_relu=False):
    D = X.shape[1]
    xs, xb = (x_pro if x_pro is not None else (None, None))
    check(lib.yolat_segment_max_fwd(_f(X), _ld(X), D, _f(xs, "x_scale", True), _f(xb, "x_shift", True),
                                    int(x_relu), g.seg_ptr.data_ptr(), g.P, g.N, _f(Y), _ld(Y),
                                    _i(arg, torch.int32, "arg"), _stream()), "yolat_segment_max_fwd")
    return Y


def segment_mean_bwd(dY, g, dX):
    D = dX.shape[1]
    check(lib.yolat_segment_mean_bwd(_f(dY), _ld(dY), D, g.seg_ptr.data_ptr(), g.node_seg.data_ptr(),
                                     g.N, _f(dX), _ld(dX), _stream()), "yolat_segment_mean_bwd")
    return dX


def segment_max_bwd(dY, arg, g, dX):
    D = dX.shape[1]
    check(lib.yolat_segment_max_bwd(_f(dY), _ld(dY), D, _i(arg, torch.int32, "arg"),
                                    g.node_seg.data_ptr(), g.N, _f(dX), _ld(dX), _stream()),
          "yolat_segment_max_bwd")
    return dX


# ---------------------------------------------------------------------------------------------
# device-side sub-batch extraction for predict()'s two passes (csrc/subgraph.hip)
# ---------------------------------------------------------------------------------------------

def _ranges_to_ids(starts, ends, dev):
    """Concatenation of range(s, e) as an int32 CUDA tensor (ranges given as host int64 arrays)."""
    import numpy as np
    lens = ends - starts
    if (lens < 0).any():
        raise ValueError("idx range with end < start")
    prefix = np.zeros(len(lens) + 1, dtype=np.int64)
    np.cumsum(lens, out=prefix[1:])
    total = int(prefix[-1])
    out = torch.empty(total, dtype=torch.int32, device=dev)
    if total:
        st = torch.from_numpy(starts.astype(np.int32)).to(dev, non_blocking=True)
        pf = torch.from_numpy(prefix.astype(np.int32)).to(dev, non_blocking=True)
        check(lib.yolat_expand_ranges(st.data_ptr(), pf.data_ptr(), len(lens), total, out.data_ptr(), _stream()),
              "yolat_expand_ranges")
        out._keep = (st, pf)
    return out


def _gather(src, idx):
    """dst[r] = src[idx[r]] for a contiguous 2-D tensor of a 4-/8-byte dtype."""
    if not src.is_contiguous() or src.dim() != 2:
        raise ValueError("gather source must be a contiguous 2-D tensor")
    rb = src.shape[1] * src.element_size()
    dst = torch.empty(idx.numel(), src.shape[1], dtype=src.dtype, device=src.device)
    check(lib.yolat_gather_rows_bytes(src.data_ptr(), rb, idx.data_ptr(), idx.numel(), rb, dst.data_ptr(), rb, _stream()),
          "yolat_gather_rows_bytes")
    return dst


def extract_subgraph(data_cls, dev_batch, pos_s, pos_e, edge_s, edge_e, slice_bbox):
    """`build_data` of arch:166-242 on the device.  dev_batch: dict of CUDA tensors x, pos, edge [E,2] int64,
    e_attr, bbox_idx int64, bbox, stat_feats.  Returns (Data of CUDA tensors, status word)."""
    import numpy as np
    x, edge, bbox_idx = dev_batch["x"], dev_batch["edge"], dev_batch["bbox_idx"]
    dev = x.device
    N = x.shape[0]
    node_ids = _ranges_to_ids(pos_s, pos_e, dev)
    edge_ids = _ranges_to_ids(edge_s, edge_e, dev)
    bbox_ids = torch.from_numpy(np.asarray(slice_bbox, dtype=np.int32)).to(dev, non_blocking=True)
    n_sub, m_sub = node_ids.numel(), edge_ids.numel()
    new = data_cls(x=_gather(x, node_ids), pos=_gather(dev_batch["pos"], node_ids))
    new.e_attr = _gather(dev_batch["e_attr"], edge_ids)
    new.bbox = _gather(dev_batch["bbox"], bbox_ids)
    new.stat_feats = _gather(dev_batch["stat_feats"], bbox_ids)
    new.edge = torch.empty(m_sub, 2, dtype=torch.int64, device=dev)
    new.bbox_idx = torch.empty(n_sub, dtype=torch.int64, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    work = torch.empty(int(lib.yolat_subgraph_work_elems(N, n_sub)), dtype=torch.int32, device=dev)
    if edge.dim() != 2 or edge.shape[1] != 2:
        raise ValueError("edge must be [E,2]")
    check(lib.yolat_subgraph_reindex(node_ids.data_ptr(), n_sub, N, _i(edge, torch.int64, "edge"), edge.stride(0),
                                     edge.stride(1), edge_ids.data_ptr(), m_sub, _i(bbox_idx, torch.int64, "bbox_idx"),
                                     new.edge.data_ptr(), new.bbox_idx.data_ptr(), work.data_ptr(), status.data_ptr(),
                                     _stream()), "yolat_subgraph_reindex")
    new._keep = (node_ids, edge_ids, bbox_ids, work)
    return new, status


# ---------------------------------------------------------------------------------------------
# training-mode fusion block + per-proposal max pooling (csrc/fusion_train.hip)
# ---------------------------------------------------------------------------------------------

def _fus_check(rc, what, A, F, bf16):
    """YOLAT_E_UNSUPPORTED of the training fusion entry points -> ValueError naming the shape and A's alignment.  The
    alignment and shape checks at entry (A 16-byte aligned, row stride % 4 == 0, K / F of the path) decline before anything
    is enqueued; the bf16 forward's GEMM can still decline an extreme N (N * F >= 2^32) after the statistics ran."""
    shape = "fusion_block A [%d, %d] (row stride %d, base address %% 16 = %d) -> %d" % (
        A.shape[0], A.shape[1], _ld(A), A.data_ptr() % 16, F)
    if bf16:
        _bt_check(rc, what, shape)
    elif rc == -2:
        raise ValueError("%s does not take %s" % (what, shape))
    check(rc, what)


def fusion_pool_train_fwd(A, lin, bn, g, Z, bf16=False):
    """Z[P,F] <- scatter_max(relu(bn(lin(A)))) with batch statistics, without materialising [N,F].
    Returns the state the backward needs.  bf16: the GEMM (and, in the backward, the sparse dA GEMM) on bf16 operands
    ("bf16_dense" training precision); the statistics stay fp32."""
    N, K = A.shape
    F = lin.out_features
    dev = A.device
    coef = torch.empty(4, F, dtype=torch.float32, device=dev)
    saved = torch.empty(int(lib.yolat_fusion_pool_train_saved_elems(K, F, g.P)), dtype=torch.float32, device=dev)
    work = torch.empty(int(lib.yolat_fusion_pool_train_work_elems(N, K, F, g.P)), dtype=torch.float32, device=dev)
    track = bn.track_running_stats and bn.running_mean is not None
    mom = 0.1 if bn.momentum is None else float(bn.momentum)
    W = lin.weight
    if not W.is_contiguous():
        raise ValueError("fusion_block weight must be contiguous")
    if track:
        bump_weight_epoch()
    fn, name = ((lib.yolat_fusion_pool_train_fwd_bf16, "yolat_fusion_pool_train_fwd_bf16") if bf16 else
                (lib.yolat_fusion_pool_train_fwd, "yolat_fusion_pool_train_fwd"))
    rc = fn(_f(A, "A"), _ld(A), N, K, _f(W), _f(lin.bias, "bias", True), F, _f(bn.weight), _f(bn.bias),
            _f(bn.running_mean if track else None, "rm", True), _f(bn.running_var if track else None, "rv", True), mom,
            float(bn.eps), g.node_seg.data_ptr(), g.P, _f(Z), _ld(Z), _f(coef), _f(saved), _f(work), _stream())
    _fus_check(rc, name, A, F, bf16)
    return {"A": A, "lin": lin, "bn": bn, "coef": coef, "saved": saved, "work": work, "bf16": bool(bf16)}


def fusion_pool_train_bwd(sv, g, gZ, dW, dbias, dgamma, dbeta, dA, side=None):
    """`side` (engine._on_side): the weight gradient (sparse gather + finish, ~140 us at cfg 3) on a second stream
    beside the input gradient; the per-column reductions both read run first on the caller's stream."""
    A, lin = sv["A"], sv["lin"]
    N, K = A.shape
    F = lin.out_features

    fn = lib.yolat_fusion_pool_train_bwd_parts_bf16 if sv.get("bf16") else lib.yolat_fusion_pool_train_bwd_parts

    def part(mask):
        rc = fn(_f(A), _ld(A), N, K, _f(lin.weight), _f(sv["bn"].weight), F, _f(sv["coef"]), _f(sv["saved"]),
                g.node_seg.data_ptr(), g.seg_ptr.data_ptr(), g.P, _f(gZ, "gZ"), _ld(gZ), _f(dW), _f(dbias, "dbias", True),
                _f(dgamma), _f(dbeta), _f(dA), _ld(dA), _f(sv["work"]), mask, _stream())
        _fus_check(rc, "yolat_fusion_pool_train_bwd_parts_bf16" if sv.get("bf16") else "yolat_fusion_pool_train_bwd",
                   A, F, sv.get("bf16"))
    if side is None:
        part(7)
        return
    part(1)
    side(lambda: part(2), (A, gZ, sv["saved"], sv["work"], sv["coef"], g.node_seg))
    part(4)


# ---------------------------------------------------------------------------------------------
# loss / optimiser
# ---------------------------------------------------------------------------------------------

def softmax_ce(logits, labels, loss, dlogits=None):
    P, K = logits.shape
    work = torch.empty(int(lib.yolat_softmax_ce_work_elems(P)), dtype=torch.float32, device=logits.device)
    check(lib.yolat_softmax_ce(_f(logits), _ld(logits), _i(labels, torch.int64, "labels"), P, K,
                               _f(loss), _f(dlogits, "dlogits", True),
                               _ld(dlogits) if dlogits is not None else K, work.data_ptr(), _stream()),
          "yolat_softmax_ce")
    return loss


def sigmoid(z, out=None):
    """out = 1 / (1 + exp(-z)) (yolat_sigmoid); `out` may be `z` itself."""
    P, K = z.shape
    if out is None:
        out = torch.empty(P, K, dtype=torch.float32, device=z.device)
    if P > 0:
        check(lib.yolat_sigmoid(_f(z, "z"), _ld(z), P, K, _f(out, "out"), _ld(out), _stream()), "yolat_sigmoid")
    return out


def sigmoid_bwd(dp, p, dz=None):
    """dz = dp * (p (1 - p)) (yolat_sigmoid_bwd)."""
    P, K = p.shape
    if dz is None:
        dz = torch.empty(P, K, dtype=torch.float32, device=p.device)
    if P > 0:
        check(lib.yolat_sigmoid_bwd(_f(dp, "dp"), _ld(dp), _f(p, "p"), _ld(p), P, K, _f(dz, "dz"), _ld(dz), _stream()),
              "yolat_sigmoid_bwd")
    return dz


def bce(prob, labels, loss, dprob=None):
    """nn.BCELoss (mean over all elements) of probabilities against one-hot labels; dprob (optional) = dLoss/dprob."""
    P, K = prob.shape
    work = torch.empty(int(lib.yolat_bce_work_elems(P)), dtype=torch.float32, device=prob.device)
    check(lib.yolat_bce(_f(prob, "prob"), _ld(prob), _i(labels, torch.int64, "labels"), P, K, _f(loss),
                        _f(dprob, "dprob", True), _ld(dprob) if dprob is not None else K, work.data_ptr(), _stream()),
          "yolat_bce")
    return loss


def sigmoid_bce(logits, labels, loss, dlogits=None, prob=None):
    """sigmoid -> bce -> sigmoid_bwd in one launch from the logits (yolat_sigmoid_bce); bit-identical to the three calls."""
    P, K = logits.shape
    work = torch.empty(int(lib.yolat_bce_work_elems(P)), dtype=torch.float32, device=logits.device)
    check(lib.yolat_sigmoid_bce(_f(logits, "logits"), _ld(logits), _i(labels, torch.int64, "labels"), P, K, _f(loss),
                                _f(dlogits, "dlogits", True), _ld(dlogits) if dlogits is not None else K,
                                _f(prob, "prob", True), _ld(prob) if prob is not None else K, work.data_ptr(), _stream()),
          "yolat_sigmoid_bce")
    return loss


def adam_step(param, grad, exp_avg, exp_avg_sq, lr, beta1, beta2, eps, weight_decay, step,
              grad_scale=1.0):
    bump_weight_epoch()
    check(lib.yolat_adam_step(_f(param), _f(grad), _f(exp_avg), _f(exp_avg_sq), param.numel(),
                              float(lr), float(beta1), float(beta2), float(eps), float(weight_decay),
                              int(step), float(grad_scale), _stream()), "yolat_adam_step")


def dropout_fwd(Y, scale, shift, relu, p, seed, Z):
    """Z = relu?(Y*scale+shift) * keep/(1-p) with an element-wise Bernoulli(1-p) mask (yolat_dropout_fwd); returns the
    uint8 mask for dropout_bwd."""
    M, C = Y.shape
    mask = torch.empty(M * C, dtype=torch.uint8, device=Y.device)
    check(lib.yolat_dropout_fwd(_f(Y), _ld(Y), M, C, _f(scale, "scale", True), _f(shift, "shift", True), int(relu),
                                float(p), int(seed), mask.data_ptr(), _f(Z), _ld(Z), _stream()), "yolat_dropout_fwd")
    return mask


def dropout_bwd(dZ, mask, p, dX):
    M, C = dZ.shape
    check(lib.yolat_dropout_bwd(_f(dZ), _ld(dZ), M, C, mask.data_ptr(), float(p), _f(dX), _ld(dX), _stream()),
          "yolat_dropout_bwd")
    return dX


def nms(boxes, scores, iou_threshold):
    """torchvision.ops.nms(boxes, scores, iou_threshold) on the HIP path (csrc/nms.hip, yolat_nms): indices of the
    kept boxes in descending score order.  boxes [n,4] (x1,y1,x2,y2), scores [n]; both CUDA tensors."""
    n = int(boxes.shape[0])
    if boxes.dim() != 2 or boxes.shape[1] != 4 or scores.dim() != 1 or scores.shape[0] != n:
        raise ValueError("nms expects boxes [n,4] and scores [n]")
    if n == 0:
        return torch.empty(0, dtype=torch.int64, device=boxes.device)
    b = boxes.detach().to(torch.float32).contiguous()
    s = scores.detach().to(torch.float32).contiguous()
    if not b.is_cuda or not s.is_cuda:
        raise ValueError("nms expects CUDA tensors")
    need = int(lib.yolat_nms_work_bytes(n))
    if need == 0:
        raise ValueError("nms supports up to 524288 boxes")
    work = torch.empty(need, dtype=torch.uint8, device=b.device)
    keep = torch.empty(n, dtype=torch.int64, device=b.device)
    cnt = torch.empty(1, dtype=torch.int32, device=b.device)
    check(lib.yolat_nms(b.data_ptr(), s.data_ptr(), n, float(iou_threshold), keep.data_ptr(), cnt.data_ptr(),
                        work.data_ptr(), work.numel(), _stream()), "yolat_nms")
    return keep[:int(cnt.item())]          # D2H sync, as torchvision's sized result implies


MAX_DET = 300          # rows of one image in det / tp (csrc/detect.hip DET_MAX_DET; train.py:45)


def _dense2(t, name, cols=None):
    """data_ptr of a contiguous 2-D fp32 CUDA tensor (optionally with a fixed number of columns)."""
    p = _f(t, name)
    if t.dim() != 2 or (cols is not None and t.shape[1] != cols) or (t.numel() > 0 and not t.is_contiguous()):
        raise ValueError("%s must be a contiguous [n, %s] tensor" % (name, "k" if cols is None else cols))
    return p


def detect_scores(logits, boxes, image_ptr, scale, softmax=True, out=None):
    """yolat_detect_scores (csrc/detect.hip): logits [R, K], boxes [R, 4], image_ptr [B + 1] int32, scale [B, 4] ->
    the evaluation loop's pred rows [R, 4 + K] = (box * scale[image], 1 - p[K-1], p[0 .. K-2]), p = softmax(logits)
    (softmax=True) or the logits themselves.  All CUDA tensors; nothing is read back."""
    lp = _f(logits, "logits")
    if logits.dim() != 2 or logits.shape[1] < 2:
        raise ValueError("detect_scores expects logits [R, K] with K >= 2")
    R, K = int(logits.shape[0]), int(logits.shape[1])
    bp = _dense2(boxes, "boxes", 4)
    ip, sp = _i(image_ptr, torch.int32, "image_ptr"), _dense2(scale, "scale", 4)
    B = int(image_ptr.shape[0]) - 1
    if boxes.shape[0] != R or B < 1 or scale.shape[0] != B:
        raise ValueError("detect_scores expects boxes [R, 4], image_ptr [B + 1] and scale [B, 4]")
    if out is None:
        out = torch.empty((R, 4 + K), dtype=torch.float32, device=logits.device)
    check(lib.yolat_detect_scores(lp, R, K, _ld(logits), bp, ip, B, sp, int(bool(softmax)), _dense2(out, "out", 4 + K),
                                  _stream()), "yolat_detect_scores")
    return out


def nms_batched_work_bytes(R, nc, B):
    """Workspace of nms_batched in bytes (0: shape not supported): linear in the R * nc candidates."""
    return int(lib.yolat_nms_batched_work_bytes(int(R), int(nc), int(B)))


def nms_batched(pred, image_ptr, conf_thres=0.25, iou_thres=0.45, agnostic=False, det=None, det_count=None):
    """yolat_nms_batched (csrc/detect.hip): the class-aware non_max_suppression of every image of a batch in one call.
    pred [R, 5 + nc] = (x1, y1, x2, y2, obj, cls...), image_ptr [B + 1] int32 -> (det [B, 300, 6], det_count [B] int32),
    both on the device; rows beyond det_count[i] are zero.  Nothing is read back."""
    pp = _dense2(pred, "pred")
    if pred.shape[1] < 6:
        raise ValueError("nms_batched expects pred [R, 5 + nc] with nc >= 1")
    R, nc = int(pred.shape[0]), int(pred.shape[1]) - 5
    ip = _i(image_ptr, torch.int32, "image_ptr")
    B = int(image_ptr.shape[0]) - 1
    if B < 1:
        raise ValueError("nms_batched expects image_ptr [B + 1] with B >= 1")
    need = nms_batched_work_bytes(R, nc, B)
    if need == 0:
        raise ValueError("nms_batched supports nc <= 4096, B <= 65536 and R * nc <= 2^27")
    dev = pred.device
    work = torch.empty(need, dtype=torch.uint8, device=dev)
    if det is None:
        det = torch.empty((B, MAX_DET, 6), dtype=torch.float32, device=dev)
    if det_count is None:
        det_count = torch.empty(B, dtype=torch.int32, device=dev)
    if tuple(det.shape) != (B, MAX_DET, 6) or not det.is_contiguous() or tuple(det_count.shape) != (B,):
        raise ValueError("nms_batched expects det [B, 300, 6] and det_count [B]")
    check(lib.yolat_nms_batched(pp, R, nc, ip, B, float(conf_thres), float(iou_thres), int(bool(agnostic)), _f(det, "det"),
                                _i(det_count, torch.int32, "det_count"), work.data_ptr(), work.numel(), _stream()),
          "yolat_nms_batched")
    return det, det_count


def detect_workspace_bytes(N, P, R, Ctot, K, B):
    """Workspace of yolat_detect in bytes (0: shape not supported)."""
    return int(lib.yolat_detect_workspace_bytes(int(N), int(P), int(R), int(Ctot), int(K), int(B)))


SEL_HEAD, SEL_STATUS = 4, 2          # yolat_predict_select's record: head words (total, tree flag, status, spare)


def sel_words(B, R_cap):
    """int32 words of that record (layout: include/yolat_hip.h): the head, B + 1 image offsets, at most R_cap rows"""
    return SEL_HEAD + B + 1 + R_cap


def sel_split(sel, B):
    """(total, tree flag, status, image_off [B + 1], rows) of a record, a device tensor or a host copy (of the head alone, too)"""
    return sel[0], sel[1], sel[SEL_STATUS], sel[SEL_HEAD:SEL_HEAD + B + 1], sel[SEL_HEAD + B + 1:]


def detect_rows(logits, bbox, sel, B, R_cap, scale, softmax=True, out=None):
    """yolat_detect_rows (csrc/detect.hip): the pred rows of the asynchronous detection from the record yolat_predict_select
    wrote.  logits [P, K], bbox [P, 4], sel [sel_words(B, R_cap)] int32, scale [B, 4] -> pred [R_cap, 4 + K]: row r < total
    equals the row ``detect_scores`` gives on ``predict``'s logits and enlarged boxes, bit for bit; the spare rows behind
    are zero.  The row count is read on the device; nothing is read back."""
    lp = _f(logits, "logits")
    if logits.dim() != 2 or logits.shape[1] < 2:
        raise ValueError("detect_rows expects logits [P, K] with K >= 2")
    P, K = int(logits.shape[0]), int(logits.shape[1])
    B, R_cap = int(B), int(R_cap)
    bp, sp = _dense2(bbox, "bbox", 4), _dense2(scale, "scale", 4)
    ip = _i(sel, torch.int32, "sel")
    if bbox.shape[0] != P or B < 1 or scale.shape[0] != B or sel.dim() != 1 or sel.numel() < sel_words(B, R_cap):
        raise ValueError("detect_rows expects bbox [P, 4], scale [B, 4] and sel [4 + B + 1 + R_cap]")
    if out is None:
        out = torch.empty((R_cap, 4 + K), dtype=torch.float32, device=logits.device)
    check(lib.yolat_detect_rows(lp, _ld(logits), P, K, bp, ip, B, R_cap, sp, int(bool(softmax)), _dense2(out, "out", 4 + K),
                                _stream()), "yolat_detect_rows")
    return out


def evaluate_workspace_bytes(N, P, R, Ctot, K, B, G, T):
    """Workspace of yolat_evaluate in bytes (0: shape not supported)."""
    return int(lib.yolat_evaluate_workspace_bytes(int(N), int(P), int(R), int(Ctot), int(K), int(B), int(G), int(T)))


def eval_rows(logits, labels, sel, B, R_cap, softmax=True):
    """yolat_eval_rows (csrc/evaluate.hip): the rows stage of the asynchronous evaluation from the record
    yolat_predict_select wrote.  logits [P, K] (the probabilities of a sigmoid model with softmax=False), labels [P] int64,
    sel [sel_words(B, R_cap)] int32 -> (loss [1] fp32, stats [2 + K * K] int32 = n_true, n_total, confusion[label, y_pred],
    y_pred [R_cap] int32, y_true [R_cap] int32), all on the device.  The loss is bit for bit DetectionLoss' on the rows
    ``predict`` gathers; entries of y_pred / y_true behind sel[0] are not written.  Nothing is read back."""
    lp = _f(logits, "logits")
    if logits.dim() != 2 or not 2 <= logits.shape[1] <= 32:
        raise ValueError("eval_rows expects logits [P, K] with K in [2, 32]")
    P, K = int(logits.shape[0]), int(logits.shape[1])
    B, R_cap = int(B), int(R_cap)
    yp, ip = _i(labels, torch.int64, "labels"), _i(sel, torch.int32, "sel")
    if labels.dim() != 1 or labels.shape[0] != P or B < 1 or sel.dim() != 1 or sel.numel() < sel_words(B, R_cap):
        raise ValueError("eval_rows expects labels [P] and sel [4 + B + 1 + R_cap]")
    dev = logits.device
    loss = torch.empty(1, dtype=torch.float32, device=dev)
    stats = torch.empty(2 + K * K, dtype=torch.int32, device=dev)
    y_pred = torch.empty(R_cap, dtype=torch.int32, device=dev)
    y_true = torch.empty(R_cap, dtype=torch.int32, device=dev)
    work = torch.empty((R_cap + 255) // 256 + 1, dtype=torch.float32, device=dev)
    check(lib.yolat_eval_rows(lp, _ld(logits), P, K, yp, ip, B, R_cap, int(bool(softmax)), stats.data_ptr(), loss.data_ptr(),
                              y_pred.data_ptr(), y_true.data_ptr(), work.data_ptr(), _stream()), "yolat_eval_rows")
    return loss, stats, y_pred, y_true


D2H_READS = 0


def d2h(t):
    """The device -> host read of the asynchronous detection path (DetectHandle.result): one synchronising copy, counted
    in ``D2H_READS`` so that a test can tell how often the path looks at the device."""
    global D2H_READS
    D2H_READS += 1
    return t.cpu()


def detect_match(det, det_count, gt_boxes, gt_labels, gt_ptr, thresholds, out=None):
    """yolat_detect_match (csrc/detect.hip): true-positive flags of get_batch_statistics for every (image, threshold)
    pair.  det [B, 300, 6] / det_count [B] as returned by nms_batched, gt_boxes [G, 4], gt_labels [G] fp32, gt_ptr [B + 1]
    int32, thresholds [T] fp32 -> tp [T, B, 300] uint8 on the device."""
    dp = _f(det, "det")
    if det.dim() != 3 or tuple(det.shape[1:]) != (MAX_DET, 6) or not det.is_contiguous():
        raise ValueError("detect_match expects det [B, 300, 6]")
    B, G, T = int(det.shape[0]), int(gt_boxes.shape[0]), int(thresholds.shape[0])
    gp, lp, tp_ = _dense2(gt_boxes, "gt_boxes", 4), _f(gt_labels, "gt_labels"), _f(thresholds, "thresholds")
    if gt_labels.dim() != 1 or gt_labels.shape[0] != G or thresholds.dim() != 1 or T < 1:
        raise ValueError("detect_match expects gt_labels [G] and thresholds [T]")
    if tuple(det_count.shape) != (B,) or tuple(gt_ptr.shape) != (B + 1,):
        raise ValueError("detect_match expects det_count [B] and gt_ptr [B + 1]")
    if out is None:
        out = torch.empty((T, B, MAX_DET), dtype=torch.uint8, device=det.device)
    if tuple(out.shape) != (T, B, MAX_DET) or out.dtype != torch.uint8 or not out.is_cuda or not out.is_contiguous():
        raise ValueError("detect_match expects out [T, B, 300] uint8 on the device")
    check(lib.yolat_detect_match(dp, _i(det_count, torch.int32, "det_count"), B, gp, lp, G, _i(gt_ptr, torch.int32, "gt_ptr"),
                                 tp_, T, out.data_ptr(), _stream()), "yolat_detect_match")
    return out


# ---------------------------------------------------------------------------------------------
# epoch metrics (csrc/metrics.hip)
# ---------------------------------------------------------------------------------------------
METRICS_BAD_GT_LABEL = 1
METRICS_MAX_THRESHOLDS = 32
METRICS_MAX_CLASSES = 32


class MetricsRecord(object):
    """The epoch record of csrc/metrics.hip: ONE uint8 device buffer ``buf`` of yolat_metrics_record_bytes(capacity_images,
    K, batch_cap) bytes and the byte offsets of its eight sections (include/yolat_hip.h: conf | cls | tp | gt_hist | stats |
    loss | batch_flags | status)."""

    __slots__ = ("buf", "capacity_images", "K", "batch_cap", "offsets", "nbytes")

    def __init__(self, buf, capacity_images, K, batch_cap):
        offs = (ctypes.c_int64 * 8)()
        n = int(lib.yolat_metrics_record_bytes(int(capacity_images), int(K), int(batch_cap), offs))
        if n == 0:
            raise ValueError("a metrics record of %d images, %d classes and %d batches is outside what csrc/metrics.hip "
                             "supports (images * 300 <= 2^27, K in [2, 32], batches <= 2^24)" % (capacity_images, K, batch_cap))
        if buf.dtype != torch.uint8 or buf.dim() != 1 or buf.numel() < n or not buf.is_contiguous():
            raise ValueError("the record buffer must be a contiguous uint8 tensor of at least %d bytes" % n)
        self.buf, self.capacity_images, self.K, self.batch_cap = buf, int(capacity_images), int(K), int(batch_cap)
        self.offsets, self.nbytes = [int(v) for v in offs], n

    def section_bytes(self):
        S, K, bc = 300 * self.capacity_images, self.K, self.batch_cap
        return [4 * S, 4 * S, 4 * S, 8 * K, 8 * (2 + K * K), 4 * bc, 8 * bc, 4]

    def section(self, i, nbytes=None):
        n = self.section_bytes()[i] if nbytes is None else int(nbytes)
        return self.buf[self.offsets[i]:self.offsets[i] + n]

    def batch_flags(self):
        """int32 view [batch_cap, 2] of the flags section: (sel[1], sel[2]) of every batch"""
        return self.section(6).view(torch.int32).view(self.batch_cap, 2)

    def _ptr(self):
        if not self.buf.is_cuda:
            raise RuntimeError("the metrics record must be a CUDA (ROCm) tensor — the yolat HIP path has no CPU fallback")
        return self.buf.data_ptr()


def metrics_record(capacity_images, K, batch_cap, device):
    """A fresh (reset) epoch record on ``device``; the reset is enqueued on the current stream."""
    if torch.device(device).type != "cuda":
        raise RuntimeError("the metrics record lives on a CUDA (ROCm) device — the yolat HIP path has no CPU fallback")
    n = int(lib.yolat_metrics_record_bytes(int(capacity_images), int(K), int(batch_cap), None))
    rec = MetricsRecord(torch.empty(max(n, 1), dtype=torch.uint8, device=device), capacity_images, K, batch_cap)
    check(lib.yolat_metrics_reset(rec._ptr(), rec.capacity_images, rec.K, rec.batch_cap, _stream()), "yolat_metrics_reset")
    return rec


def metrics_grow(rec, capacity_images, batch_cap):
    """A larger record with ``rec``'s content: allocate, reset, device copies of the sections — all on the current stream,
    nothing read back.  The caller orders the streams that still write ``rec`` in front of this one and swaps."""
    if capacity_images < rec.capacity_images or batch_cap < rec.batch_cap:
        raise ValueError("metrics_grow only grows")
    rec._ptr()
    new = metrics_record(capacity_images, rec.K, batch_cap, rec.buf.device)
    for i, n in enumerate(rec.section_bytes()):
        new.section(i, n).copy_(rec.section(i, n))
    return new


def _metrics_batch(det, det_count, tp, stats, loss, gt_labels, K):
    dp = _f(det, "det")
    if det.dim() != 3 or tuple(det.shape[1:]) != (MAX_DET, 6) or not det.is_contiguous() or det.shape[0] < 1:
        raise ValueError("metrics_append expects det [B, 300, 6]")
    B = int(det.shape[0])
    cp, sp, lp = _i(det_count, torch.int32, "det_count"), _i(stats, torch.int32, "stats"), _f(loss, "loss")
    if not tp.is_cuda:
        raise RuntimeError("tp must be a CUDA (ROCm) tensor — the yolat HIP path has no CPU fallback")
    if tp.dtype != torch.uint8 or tp.dim() != 3 or tuple(tp.shape[1:]) != (B, MAX_DET) or not tp.is_contiguous():
        raise ValueError("metrics_append expects tp [T, B, 300] uint8")
    T = int(tp.shape[0])
    if not 1 <= T <= METRICS_MAX_THRESHOLDS:
        raise ValueError("metrics_append takes 1 to 32 thresholds, one bit of a slot's mask each")
    if tuple(det_count.shape) != (B,) or tuple(stats.shape) != (2 + K * K,) or loss.numel() < 1:
        raise ValueError("metrics_append expects det_count [B], stats [2 + K * K] and loss [1]")
    gp = _f(gt_labels, "gt_labels")
    if gt_labels.dim() != 1:
        raise ValueError("metrics_append expects gt_labels [G]")
    G = int(gt_labels.shape[0])
    return dp, cp, tp.data_ptr(), sp, lp, (gp if G > 0 else None), G, B, T


def metrics_append(rec, det, det_count, tp, stats, loss, gt_labels, sel, image_base, batch_index):
    """yolat_metrics_append (csrc/metrics.hip): ONE launch on the current stream that appends what yolat_evaluate wrote for
    a batch — det [B, 300, 6], det_count [B], tp [T, B, 300] uint8, stats [2 + K * K] int32, loss [1], sel — and the batch's
    target classes gt_labels [G] fp32 to the record: the images take the slots of image_base .. image_base + B - 1, the
    batch is number batch_index.  sel[1] / sel[2] are read on the device; nothing is read back."""
    rp = rec._ptr()
    a = _metrics_batch(det, det_count, tp, stats, loss, gt_labels, rec.K)
    if sel is None or sel.dim() != 1 or sel.numel() < 4:
        raise ValueError("metrics_append expects the sel record of yolat_predict_select (at least its four head words)")
    check(lib.yolat_metrics_append(rp, rec.capacity_images, rec.K, rec.batch_cap, a[0], a[1], a[2], a[3], a[4], a[5], a[6],
                                   _i(sel, torch.int32, "sel"), a[7], a[8], int(image_base), int(batch_index), _stream()),
          "yolat_metrics_append")


def metrics_append_host(rec, det, det_count, tp, stats, loss, gt_labels, image_base, batch_index):
    """yolat_metrics_append_host: ``metrics_append`` for a batch the HOST evaluated (the synchronous fall-back) and
    uploaded — no sel, the batch's flags stay as the device stored them."""
    rp = rec._ptr()
    a = _metrics_batch(det, det_count, tp, stats, loss, gt_labels, rec.K)
    check(lib.yolat_metrics_append_host(rp, rec.capacity_images, rec.K, rec.batch_cap, a[0], a[1], a[2], a[3], a[4], a[5],
                                        a[6], a[7], a[8], int(image_base), int(batch_index), _stream()),
          "yolat_metrics_append_host")


def metrics_finalize(rec, n_images, n_batches, T):
    """yolat_metrics_finalize over the first n_images images and n_batches batches of the record -> the out block as ONE
    int64 device tensor (``metrics_unpack`` names its parts on the host).  Nothing is read back."""
    rp = rec._ptr()
    n_images, n_batches, T = int(n_images), int(n_batches), int(T)
    need = int(lib.yolat_metrics_finalize_work_bytes(n_images, T, rec.K))
    nout = int(lib.yolat_metrics_out_bytes(T, rec.K, n_batches))
    if need == 0 or nout == 0:
        raise ValueError("metrics_finalize supports 1 to 32 thresholds, K in [2, 32] and 1 to 447392 images")
    dev = rec.buf.device
    work = torch.empty(need, dtype=torch.uint8, device=dev)
    out = torch.empty(nout // 8, dtype=torch.int64, device=dev)
    check(lib.yolat_metrics_finalize(rp, rec.capacity_images, rec.K, rec.batch_cap, n_images, n_batches, T, out.data_ptr(),
                                     nout, work.data_ptr(), need, _stream()), "yolat_metrics_finalize")
    return out


def metrics_unpack(words, T, K, n_batches):
    """The host copy (numpy int64) of ``metrics_finalize``'s block -> dict: ap / p / r [T, K] float64, n_gt / n_p [K],
    loss_mean, stats [2 + K * K], status, batch_flags [n_batches, 2] int32."""
    import numpy as np
    w = np.ascontiguousarray(words, dtype=np.int64)
    TK, o = T * K, 0
    out = {}
    for name in ("ap", "p", "r"):
        out[name] = w[o:o + TK].view(np.float64).reshape(T, K).copy()
        o += TK
    out["n_gt"], out["n_p"] = w[o:o + K].copy(), w[o + K:o + 2 * K].copy()
    o += 2 * K
    out["loss_mean"] = float(w[o:o + 1].view(np.float64)[0])
    out["stats"] = w[o + 1:o + 3 + K * K].copy()
    o += 3 + K * K
    out["status"] = int(w[o])
    out["batch_flags"] = w[o + 1:o + 1 + n_batches].view(np.int32).reshape(n_batches, 2).copy()
    return out
