"""Eval-mode fast path: SparseCADGCN.forward as ONE call into libyolat_hip.so (yolat_forward_eval).

``EvalPlan`` folds every BatchNorm1d into per-channel (scale, shift) once per weight version, fills
the ``yolat_model_eval`` descriptor with device pointers and owns a grow-only workspace.  Each forward
is then a single ctypes call; the C++ side enqueues graph pre-processing and all layers back to back.
"""
import ctypes
import operator
import os

import torch

from . import ops
import weakref

from ._lib import lib, check, ModelEval, ModelEvalBf16, GraphCsr, Locality, YOLAT_MAX_LAYERS

# skip the memset of the CSR-build counters when the plan's workspace was last used by a forward of the same shape
# (yolat_forward_eval_primed, include/yolat_hip.h); module flag, False: always the self-contained call
# (tests/test_gpu_model.py runs both)
PRIMED_WS = True

# bf16 plan: all conv layers + the pooling prologue in ONE launch for proposal-local batches (csrc/conv_local.hip; the
# per-layer launches stay enqueued as its gated fall-back).  False: the per-layer launches only.
CONV_LOCAL = True

# bf16 plan: examine a resident batch once per batch version (yolat_batch_locality: one extra launch pair + one host read)
# so that a proposal-local batch runs WITHOUT the global COO -> CSR build and without the gated fall-back launches, and an
# unfit one goes straight to the per-layer path.  False: every forward finds out on the device (the gated form).
LOCALITY_CACHE = True


def _x6_on(default=True):
    """A bf16x6-emulated stage of the fp32 plan: off as a whole under YOLAT_STRICT_FP32=1 (csrc/x6.hpp: strict IEEE
    propagation / fp32 MFMA summation order) — the one switch; `default` False = a stage that measured no faster than its
    fp32-MFMA form and stays off."""
    if os.environ.get("YOLAT_STRICT_FP32", "0") == "1":
        return False
    return bool(default)


def _ptr(t):
    if t.dtype != torch.float32 or not t.is_cuda or not t.is_contiguous():
        raise ValueError("model tensors must be contiguous fp32 CUDA tensors")
    return t.data_ptr()


# The helpers below append every tensor they create to `keep`: the descriptor holds addresses only.

def _lin_bn(lin, bn, dev, keep):
    """A Linear and the eval-mode BatchNorm1d behind it: the addresses (W, b, scale, shift) and the fold itself, the
    BatchNorm as per-channel coefficients [2, C] = (scale, shift)."""
    W, b = _ptr(lin.weight), _ptr(lin.bias)
    fold = torch.empty(2, bn.num_features, dtype=torch.float32, device=dev)
    ops.bn_eval_coeffs(bn, fold[0], fold[1])
    keep.append(fold)
    return (W, b, fold[0].data_ptr(), fold[1].data_ptr()), fold


def _shift(lin, fold, keep):
    """Bias of a Linear and the folded BatchNorm behind it as one vector: s * b + t (fold None: b; no bias: b = 0)."""
    b = lin.bias.detach() if lin.bias is not None else torch.zeros(lin.out_features, device=lin.weight.device)
    t = (fold[0] * b + fold[1]).contiguous() if fold is not None else b.float().contiguous()
    keep.append(t)
    return t


def _split3(w, row_scale, packed, keep):
    """Exact 3-way bfloat16 split of a weight [rows, cols] for a bf16x6-emulated kernel, rows scaled first when row_scale
    is given (a folded BatchNorm).  Addresses of the three planes, or of the one packed image of the skinny kernel."""
    rows, cols = w.shape
    scale = row_scale.data_ptr() if row_scale is not None else None
    if packed:
        parts = [torch.empty(lib.yolat_split_bf16x3_packed_elems(rows, cols), dtype=torch.bfloat16, device=w.device)]
        check(lib.yolat_split_bf16x3_packed(_ptr(w), cols, rows, cols, scale, parts[0].data_ptr(), ops._stream()),
              "yolat_split_bf16x3_packed")
    else:
        _ptr(w)
        parts = ops.split_bf16x3(w, row_scale)
    keep.extend(parts)
    return [p.data_ptr() for p in parts]


_VERSION_OF = operator.attrgetter("_version")


def rownorm_bf16_operands(lin):
    """What the bf16 plan hands k_hfusion_rows8_rn (csrc/fusion_h8_rn.hip) for a Linear [F, D] behind a row norm: the weight
    centred over its F outputs in float64, Wc = W - mean_rows(W), rounded to bf16 (round to nearest even), and the centred bias
    in fp32 (ops.rownorm_center).  Pure torch: runs wherever the weight lives."""
    wc, bc = ops.rownorm_center(lin.weight, lin.bias)
    return wc.to(torch.bfloat16).contiguous(), bc


class EvalPlan(object):
    """precision: "fp32" (default) or "bf16" — bf16 STORAGE of the node activations / weights with fp32
    accumulation (csrc/bf16_eval.hip, yolat_forward_eval_bf16), the mode of the large-graph configuration.
    row_norm: the opt-in of the bf16 plan for a norm = layer / instance model (SparseCADGCN.set_eval_precision)."""

    def __init__(self, model, precision="fp32", row_norm=False):
        if precision not in ("fp32", "bf16"):
            raise ValueError("precision must be 'fp32' or 'bf16'")
        from .engine import model_norm
        if precision != "fp32" and not row_norm and model_norm(model) != "batch":
            raise ValueError("the %s eval plan runs norm = %s only when asked to (row_norm=True)"
                             % (precision, model_norm(model)))
        self.precision = precision
        self._desc_h = None
        self.model = model
        # (PReLU slopes are not part of the weight version: the kernels read them through their address, so an in-place
        # edit neither rebuilds the descriptor nor drops a captured graph)
        slopes = set(id(p) for mod in model.modules() if isinstance(mod, torch.nn.PReLU) for p in mod.parameters())
        self._tensors = [t for t in model.parameters() if id(t) not in slopes] + [b for b in model.buffers()]
        self._key = None
        self._desc = None
        self._keep = None
        self._ws = None
        self._status = None
        self._graphs = {}
        self._need = {}           # (N, E, P, descriptor build) -> workspace bytes
        self._primed = None        # (workspace, descriptor build, N, E, P, stream) of the last completed direct launch
        self._desc_key = 0
        self._loc = {}             # batch version -> (weakrefs, Locality): the locality property, examined once
        self.use_graph = False      # model.use_hip_graphs(True) turns the captured-graph replay on

    def _version_key(self):
        return tuple(map(_VERSION_OF, self._tensors)) + (self._tensors[0].data_ptr(), ops.weight_epoch())

    def _build(self):
        self._desc_key += 1
        self._primed = None
        from .engine import model_convs
        m, net = self.model, self.model.cls_net
        dev = self._tensors[0].device
        convs = model_convs(net)
        if len(convs) > YOLAT_MAX_LAYERS:
            raise ValueError("n_blocks > %d is not supported by the eval plan" % YOLAT_MAX_LAYERS)
        d = ModelEval()
        keep = []
        d.n_blocks, d.n_blocks_out, d.n_classes = net.n_blocks, net.n_blocks_out, m.n_classes
        d.C = convs[0].nn[0].out_features
        d.F = net.fusion_block[0].out_features
        layers = [self._build_conv(d.conv[l], l, cv, dev, keep) for l, cv in enumerate(convs)]
        ff, ffs = self._build_head(d, dev, keep)
        self._desc, self._keep = d, keep
        self._desc_h = None
        if self.precision == "bf16":
            self._desc_h = self._build_bf16(d, convs, layers, ff, ffs, dev, keep)
        if self._status is None:
            self._status = torch.zeros(1, dtype=torch.int32, device=dev)

    def _build_conv(self, c, l, cv, dev, keep):
        """Entry `c` of conv layer l.  Returns (Wuv, fold of nn.1, fold of nn.4): what the bf16 descriptor starts from."""
        C, cin = cv.nn[0].out_features, cv.in_channels
        c.Cin = cin
        (c.W1, c.b1, c.s1, c.t1), f1 = _lin_bn(cv.nn[0], cv.nn[1], dev, keep)
        (c.W2, c.b2, c.s2, c.t2), f2 = _lin_bn(cv.nn[3], cv.nn[4], dev, keep)
        c.Wr, c.br = _ptr(cv.lin_r.weight), _ptr(cv.lin_r.bias)
        (c.Wn, c.bn, c.sn, c.tn), fn = _lin_bn(cv.mlp_node[0], cv.mlp_node[1], dev, keep)
        # factorised first edge Linear: per-node weights [W1a - W1b | W1b] and the 4 attr columns
        wuv, wc4 = ops.split_w1(cv.nn[0].weight, cin)
        keep += [wuv, wc4]
        c.Wuv, c.Wc4 = wuv.data_ptr(), wc4.data_ptr()
        if self.precision != "fp32":
            return wuv, f1, f2
        # folded form of the layer (once per weight version; elementwise on [C]-sized tensors): nn.1's folded BatchNorm
        # (s1, t1) and the bias b1 move into the per-node products and the attr weights, b2 into the shift of nn.4 — the
        # per-edge arithmetic shrinks to
        #   h1 = relu(U'[dst] + V'[src] + Wc4f.attr),  message = relu(s2 * (W2.h1) + t2f)
        wuvf, uvb, wc4f, t2f = ops.fold_factorised_layer(wuv, wc4, cv.nn[0].bias, f1[0], f1[1], cv.nn[3].bias, f2[0], f2[1])
        keep += [wuvf, uvb, wc4f, t2f]
        c.Wuvf, c.uvb, c.Wc4f, c.t2f = wuvf.data_ptr(), uvb.data_ptr(), wc4f.data_ptr(), t2f.data_ptr()
        stacked = cin == 64 and C == 64 and cv.lin_r.bias is not None
        chain = l > 0 and stacked and os.environ.get("YOLAT_NODE_CHAIN", "1") != "0"
        rows_x6 = stacked and _x6_on()
        if chain or rows_x6:
            # the node side as one product: [Wuvf ; Wr] stacked, shifts [uvb ; br]
            wfr = torch.cat([wuvf, cv.lin_r.weight.detach()], 0)                           # [192, 64]
            tfr = torch.cat([uvb, cv.lin_r.bias.detach()], 0)
            keep += [wfr, tfr]
        if chain:
            # ... in the form the PREVIOUS layer's edge kernel consumes (small graphs: EdgeNext, csrc/internal.hpp):
            # the weight in 16x16x4 MFMA B-fragment order
            wnx = wfr.view(12, 16, 16, 4).permute(0, 2, 3, 1).contiguous()                 # [ct, ks, k & 3, row]
            keep.append(wnx)
            c.Wnx, c.tnx = wnx.data_ptr(), tfr.data_ptr()
        if rows_x6:
            # ... on the bf16x6 rows kernel (yolat_node_uv_eval_x6): the weight split; the node branch with its BatchNorm
            # scale folded into the weight rows
            c.Wfr_x6[0], c.Wfr_x6[1], c.Wfr_x6[2] = _split3(wfr, None, False, keep)
            c.Wn_x6[0], c.Wn_x6[1], c.Wn_x6[2] = _split3(cv.mlp_node[0].weight, fn[0], False, keep)
            c.tfr, c.tn_fold = tfr.data_ptr(), _shift(cv.mlp_node[0], fn, keep).data_ptr()
        return wuv, f1, f2

    def _build_head(self, d, dev, keep):
        """The two fusion blocks and the classifier.  Returns the folds of the two fusion BatchNorms."""
        m, net = self.model, self.model.cls_net
        fp32 = self.precision == "fp32"
        fb, fs = net.fusion_block, net.fusion_block_super
        # the activation of the four sites behind the conv stack (csrc/act.hip).  The descriptor holds the ADDRESS of each
        # slope — a PReLU weight itself, or a constant cached on the LeakyReLU module — so an in-place edit needs no rebuild
        # and is seen by a hipGraph replay; ReLU leaves the fields zero
        from .engine import model_act
        acts = model_act(m)
        kinds = set(ops.act_kind(a) for a in acts if a is not True)
        if any(a is False for a in acts) or len(kinds) > 1:
            raise NotImplementedError("the eval plan needs one act (relu, leakyrelu or prelu) at all four sites")
        if kinds:
            d.act = kinds.pop()
            for i, a in enumerate(acts):
                t = ops.act_slope(a, dev)
                keep.append(t)
                d.act_slope[i] = t.data_ptr()
        from .engine import model_norm
        if model_norm(m) != "batch":
            return self._build_head_rownorm(d, dev, keep, bool(kinds))
        (d.Wf, d.bf, d.sf, d.tf), ff = _lin_bn(fb[0], fb[1], dev, keep)
        (d.Wfs, d.bfs, d.sfs, d.tfs), ffs = _lin_bn(fs[0], fs[1], dev, keep)
        # Linear + BatchNorm for the bf16x6-emulated fusion kernel: BatchNorm scale folded into the weight rows, exact 3-way
        # bfloat16 split of the result, shift = s*b + t
        if fp32 and _x6_on() and fb[0].in_features in (64, 128) and d.F % 64 == 0:
            d.Wf_hi, d.Wf_mid, d.Wf_lo = _split3(fb[0].weight, ff[0], False, keep)
            d.tf_fold = _shift(fb[0], ff, keep).data_ptr()
            d.Wfs_hi, d.Wfs_mid, d.Wfs_lo = _split3(fs[0].weight, ffs[0], False, keep)
            d.tfs_fold = _shift(fs[0], ffs, keep).data_ptr()
            # ... and for its f16x3 form (csrc/f16x3.hpp): the same scaled rows as two half-precision planes and one scale
            # exponent per row; the forward picks the launch (YOLAT_FUSION_F16X3)
            for lin, fold, planes, exp_name in ((fb[0], ff, d.Wf_f16, "Wf_exp"), (fs[0], ffs, d.Wfs_f16, "Wfs_exp")):
                _ptr(lin.weight)
                hi, lo, exps = ops.split_f16x2(lin.weight, fold[0])
                keep += [hi, lo, exps]
                planes[0], planes[1] = hi.data_ptr(), lo.data_ptr()
                setattr(d, exp_name, exps.data_ptr())
        m1, m2, m3 = m.prediction_cls[0], m.prediction_cls[1], m.prediction_cls[2]
        d.H1, d.H2 = m1[0].out_features, m2[0].out_features
        (d.Wc1, d.bc1, d.sc1, d.tc1), fc1 = _lin_bn(m1[0], m1[1], dev, keep)
        (d.Wc2, d.bc2, d.sc2, d.tc2), fc2 = _lin_bn(m2[0], m2[1], dev, keep)
        d.Wc3, d.bc3 = _ptr(m3[0].weight), _ptr(m3[0].bias)
        # prediction_cls.0 (P x 2304 -> 512) on the LDS-tiled bf16x6 GEMM (yolat_gemm_x6)
        if fp32 and _x6_on() and m1[0].in_features % 16 == 0:
            rows, cols = m1[0].out_features, m1[0].in_features
            packed = torch.empty(lib.yolat_gemm_x6_packed_elems(rows, cols), dtype=torch.bfloat16, device=dev)
            check(lib.yolat_gemm_x6_pack(_ptr(m1[0].weight), cols, rows, cols, fc1[0].data_ptr(), packed.data_ptr(),
                                         ops._stream()), "yolat_gemm_x6_pack")
            keep.append(packed)
            d.Wc1_gx, d.tc1_gx = packed.data_ptr(), _shift(m1[0], fc1, keep).data_ptr()
        # classifier layers for the skinny bf16x6 kernel (yolat_linear_x6): all three or none.  Off by default: measured
        # equal to the fp32 split-K kernel at P = 400 (20.8 vs 21.2 us for cls1; operands streamed from L2 straight
        # into registers make it L1-bandwidth bound, profiles/r02_linear_x6_skinny.txt) and slower beyond.
        if fp32 and _x6_on(False) and all(l[0].in_features % 16 == 0 for l in (m1, m2, m3)):
            for i, (lin, fold) in enumerate(((m1[0], fc1), (m2[0], fc2), (m3[0], None))):
                d.Wc_x6[i] = _split3(lin.weight, fold[0] if fold is not None else None, True, keep)[0]
                d.tc_fold[i] = _shift(lin, fold, keep).data_ptr()
        return ff, ffs

    def _build_head_rownorm(self, d, dev, keep, leaky):
        """_build_head for norm = layer / instance (csrc/rownorm.hip): a row norm does not fold into its Linear, so the
        descriptor carries plain weights and biases (the BatchNorm scale / shift fields stay NULL and are not read), the
        LayerNorm weight / bias of each site by ADDRESS, and for the fused fusion kernel the split of the weights centred over
        their outputs (ops.rownorm_center) with the centred bias.  As the base of a bf16 plan (row_norm=True) it carries the
        addresses, gamma / beta / eps and the route with the opt-in bit; the centred bf16 weights are _build_bf16's."""
        m, net = self.model, self.model.cls_net
        if leaky:
            raise NotImplementedError("norm = layer / instance with act = leakyrelu / prelu has no MI355X kernel")
        fb, fs = net.fusion_block, net.fusion_block_super
        m1, m2, m3 = m.prediction_cls[0], m.prediction_cls[1], m.prediction_cls[2]
        sites = (fb, fs, m1, m2)
        d.norm = ops.norm_kind(sites[0][1])
        eps = set()
        for i, blk in enumerate(sites):
            gamma, beta, e = ops.rownorm_params(blk[1])
            eps.add(e)
            if gamma is not None:
                d.rn_gamma[i], d.rn_beta[i] = _ptr(gamma), _ptr(beta)
        if len(eps) != 1:
            raise NotImplementedError("the eval plan needs one eps at all four norm sites, got %s" % sorted(eps))
        d.rn_eps = eps.pop()
        # which fusion-pair route: by the node count unless YOLAT_RN_FUSED=1 | 0 names one — read HERE, once
        # per descriptor build, so a plan's workspace sizing and its forwards cannot disagree (the tests and
        # tools/rownorm_ab.py run both routes on one graph)
        d.rn_route = {"1": ops.RN_ROUTE_FUSED, "0": ops.RN_ROUTE_MATERIALISE}.get(os.environ.get("YOLAT_RN_FUSED", ""),
                                                                                   ops.RN_ROUTE_AUTO)
        d.Wf, d.bf = _ptr(fb[0].weight), _ptr(fb[0].bias)
        d.Wfs, d.bfs = _ptr(fs[0].weight), _ptr(fs[0].bias)
        fp32 = self.precision == "fp32"
        if not fp32:
            # the base of a bf16 descriptor: the opt-in travels in rn_route (YOLAT_RN_ROUTE_BF16); the bf16x6 operand forms
            # below are the fp32 forward's and are not made (_build_bf16 makes the bf16 ones)
            d.rn_route |= ops.RN_ROUTE_BF16
        if fp32 and _x6_on() and fb[0].in_features in (64, 128) and d.F % 64 == 0:
            for lin, names in ((fb[0], ("Wf_hi", "Wf_mid", "Wf_lo", "tf_fold")), (fs[0], ("Wfs_hi", "Wfs_mid", "Wfs_lo", "tfs_fold"))):
                wc, bc = ops.rownorm_center(lin.weight, lin.bias)
                keep += [wc, bc]
                hi, mid, lo = _split3(wc, None, False, keep)
                for n, v in zip(names, (hi, mid, lo, bc.data_ptr())):
                    setattr(d, n, v)
        d.H1, d.H2 = m1[0].out_features, m2[0].out_features
        d.Wc1, d.bc1 = _ptr(m1[0].weight), _ptr(m1[0].bias)
        d.Wc2, d.bc2 = _ptr(m2[0].weight), _ptr(m2[0].bias)
        d.Wc3, d.bc3 = _ptr(m3[0].weight), _ptr(m3[0].bias)
        # prediction_cls.0 on the LDS-tiled bf16x6 GEMM (yolat_gemm_x6): packed without a row scale, shift = bias
        if fp32 and _x6_on() and m1[0].in_features % 16 == 0:
            rows, cols = m1[0].out_features, m1[0].in_features
            packed = torch.empty(lib.yolat_gemm_x6_packed_elems(rows, cols), dtype=torch.bfloat16, device=dev)
            check(lib.yolat_gemm_x6_pack(_ptr(m1[0].weight), cols, rows, cols, None, packed.data_ptr(), ops._stream()),
                  "yolat_gemm_x6_pack")
            keep.append(packed)
            d.Wc1_gx, d.tc1_gx = packed.data_ptr(), _shift(m1[0], None, keep).data_ptr()
        return None, None

    def _build_bf16(self, d, convs, layers, ff, ffs, dev, keep):
        """The bf16-storage descriptor on top of `d`, from the folds computed for it (layers: _build_conv's results)."""
        m, net = self.model, self.model.cls_net
        h = ModelEvalBf16()
        h.base = ctypes.pointer(d)

        def half(t):
            o = torch.empty(t.numel(), dtype=torch.bfloat16, device=dev)
            check(lib.yolat_f32_to_bf16(t.data_ptr(), t.numel(), o.data_ptr(), ops._stream()), "yolat_f32_to_bf16")
            keep.append(o)
            return o.data_ptr()

        def half_folded(lin, fold):
            # BatchNorm scale folded into the weight rows before the bf16 rounding; its shift + the bias go as one vector
            return half((lin.weight.detach() * fold[0][:, None]).contiguous()), _shift(lin, fold, keep).data_ptr()

        for l, (cv, (wuv, f1, f2)) in enumerate(zip(convs, layers)):
            # the edge MLP's second BatchNorm (the vector enters the accumulators through an MFMA, csrc/edge_chain.hip)
            h.W2[l], h.t2f[l] = half_folded(cv.nn[3], f2)
            # layer 1's folded BatchNorm moves into the node-side epilogue: U' = s1*U + (s1*b1 + t1), V' = s1*V
            uvs = torch.cat([f1[0], f1[0]]).contiguous()
            uvt = torch.cat([_shift(cv.nn[0], f1, keep), torch.zeros_like(f1[1])]).contiguous()
            keep += [uvs, uvt]
            h.uv_scale[l], h.uv_shift[l] = uvs.data_ptr(), uvt.data_ptr()
            if l > 0:
                h.Wuv[l], h.Wr[l], h.Wn[l] = half(wuv), half(cv.lin_r.weight), half(cv.mlp_node[0].weight)
        fb, fs = net.fusion_block, net.fusion_block_super
        h.Wf, h.Wfs = half(fb[0].weight), half(fs[0].weight)
        if d.norm != ops.NORM_BATCH:
            # a row norm has nothing to fold: the fold slots carry the weights CENTRED over their outputs and the centred bias,
            # the operands of the fused row-norm kernel (csrc/fusion_h8_rn.hip); the plain Wf / Wfs serve the materialising route
            for lin, wname, tname in ((fb[0], "Wf_fold", "tf_fold"), (fs[0], "Wfs_fold", "tfs_fold")):
                wc, bc = rownorm_bf16_operands(lin)
                keep += [wc, bc]
                setattr(h, wname, wc.data_ptr())
                setattr(h, tname, bc.data_ptr())
        else:
            # the two fusion blocks with their BatchNorm folded: the A-in-registers rows kernel, csrc/fusion_h8.hip
            h.Wf_fold, h.tf_fold = half_folded(fb[0], ff)
            h.Wfs_fold, h.tfs_fold = half_folded(fs[0], ffs)
        h.Wc1, h.Wc2, h.Wc3 = (half(m.prediction_cls[i][0].weight) for i in range(3))
        # the conv stack's weights in the fragment order of the one-launch proposal-local kernel (csrc/conv_local.hip);
        # models outside its shapes (C != 64, in_channels > 8) keep the per-layer launches
        if CONV_LOCAL:
            nbytes = int(lib.yolat_conv_local_pack_bytes(d.n_blocks))
            pack = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            rc = lib.yolat_conv_local_pack(ctypes.byref(h), pack.data_ptr(), nbytes, ops._stream())
            if rc == 0:
                keep.append(pack)
                h.conv_local = pack.data_ptr()
            elif rc != -2:        # YOLAT_E_UNSUPPORTED: shapes the kernel is not written for
                check(rc, "yolat_conv_local_pack")
        return h

    def _local_candidate(self, P):
        """would yolat_forward_eval_bf16 consider the one-launch conv stack for a batch of P proposals?  (the model's
        shapes packed, YOLAT_CONV_LOCAL — read per call like the C side does — and its P >= 1024 rule)"""
        if self._desc_h is None or not self._desc_h.conv_local:
            return False
        mode = os.environ.get("YOLAT_CONV_LOCAL", "1")
        return mode != "0" and (mode in ("2", "3") or P >= 1024)

    def _vouched(self, loc, P):
        return (loc is not None and self._local_candidate(P) and
                lib.yolat_conv_local_fits(ctypes.byref(loc), P) != 0)

    def locality(self, edge, bbox_idx, N, E, P, se, sc):
        """The batch's locality record (yolat_locality), examined on the device ONCE per batch version: the key is the
        identity, storage address and `_version` of the two index tensors — the invalidation rule of the model's stage
        cache, so an in-place edit (`edge[5, 0] = ...`) is seen.  The record holds weak references to the tensors it
        was taken from: an address recycled for another tensor never matches.  Returns None when the one-launch conv
        stack is not a candidate for this model / batch size (nothing to decide: no examination, no host read)."""
        if not LOCALITY_CACHE or not self._local_candidate(P):
            return None
        key = (id(edge), edge.data_ptr(), edge._version, id(bbox_idx), bbox_idx.data_ptr(), bbox_idx._version, N, E, P, se, sc)
        ent = self._loc.get(key)
        if ent is not None and ent[0]() is edge and ent[1]() is bbox_idx:
            return ent[2]
        need = int(lib.yolat_batch_locality_workspace_bytes(N, E, P))
        ws = torch.empty(need + 16, dtype=torch.uint8, device=bbox_idx.device)
        info = torch.empty(4, dtype=torch.int32, device=bbox_idx.device)
        check(lib.yolat_batch_locality(ops._i(edge, torch.int64, "edge") if E > 0 else None, se, sc,
                                       ops._i(bbox_idx, torch.int64, "bbox_idx"), N, E, P, info.data_ptr(), ws.data_ptr(),
                                       ws.numel(), ops._stream()), "yolat_batch_locality")
        flags, mn, me, bad = info.tolist()             # the one host read per batch version
        loc = Locality(1, int(flags) | (4 if bad else 0), int(mn), int(me))
        if len(self._loc) >= 16:
            self._loc.pop(next(iter(self._loc)))
        self._loc[key] = (weakref.ref(edge), weakref.ref(bbox_idx), loc)
        return loc

    def _prepare(self, N, E, P):
        """The common opening of every forward: the descriptor of the current weight version and a workspace (grow-only)
        large enough for the shape.  A rebuild or a new workspace drops the captured graphs."""
        key = self._version_key()
        if key != self._key:
            self._build()
            self._key = key
            self._graphs.clear()
        nk = (N, E, P, self._desc_key)
        need = self._need.get(nk)
        if need is None:
            if self._desc_h is not None:
                need = int(lib.yolat_forward_eval_bf16_workspace_bytes(ctypes.byref(self._desc_h), N, E, P))
            else:
                need = int(lib.yolat_forward_eval_workspace_bytes(ctypes.byref(self._desc), N, E, P))
            if len(self._need) > 64:
                self._need.clear()
            self._need[nk] = need
        if self._ws is None or self._ws.numel() < need:
            self._ws = torch.empty(int(need * 1.25) + 4096, dtype=torch.uint8, device=self._tensors[0].device)
            self._graphs.clear()

    def run(self, x, edge, e_attr, bbox_idx, num_proposals, loc=None):
        """loc: the batch's locality record when the caller has it (decided on the host by the collate); None: the plan
        examines a resident batch itself, once per batch version (`locality`)"""
        N, P = x.shape[0], int(num_proposals)
        E, se, sc = ops.edge_layout(edge)
        self._prepare(N, E, P)
        if self.use_graph:
            out = self._run_graph(x, edge, e_attr, bbox_idx, N, E, P, se, sc)
            if out is not None:
                return out
        return self._launch(x, edge, e_attr, bbox_idx, N, E, P, se, sc, loc)

    def run_raw(self, raw, loc=None):
        """The forward on a DeviceLoader batch in COO mode, described by addresses instead of tensor views:
        raw = (x, ldx, edge, stride_e, stride_c, e_attr, bbox_idx, N, E, P, device) — every tensor view costs this thread
        what a launch costs, and the hand-over is bound by exactly that (data.DeviceLoader)."""
        xp, ldx, ep, se, sc, ap, bp, N, E, P, dev = raw
        self._prepare(N, E, P)
        return self._launch_coo(xp, ldx, ep, se, sc, ap, bp, N, E, P, dev, loc, False)

    def run_prepared(self, x, g, xref=None, loc=None):
        """The forward on a prepared device graph (ops.Graph; yolat_forward_eval_csr / _bf16_loc): no COO -> CSR
        conversion inside the call.  (hipGraph replay of this path was measured and dropped twice: batches arrive in fresh
        allocations, so captured graphs rarely match — 4.3 k vs 6.2 k graphs/s H2D-inclusive at cfg 2, round 3; keyed by the
        fixed slot addresses of a data.DeviceLoader ring they do match, and replay + the copy out of the static output
        still lose to seven direct launches — 7.3 k vs 7.9 k graphs/s, round 5.)
        xref = (address, row stride, rows, device) of a dense fp32 x that exists only as a range of a loader slot
        (data.DeviceLoader): the hand-over is bound by this thread's Python, a tensor view costs what a launch costs"""
        N, E, P = g.N, g.E, g.P
        self._prepare(N, E, P)
        self._primed = None
        gc = GraphCsr(*g.device_pointers())
        if xref is not None:
            xp, ldx, rows, dev = xref
            if rows != N:
                raise ValueError("x has %d rows, the prepared graph %d nodes" % (rows, N))
        else:
            xp, ldx, dev = ops._f(x, "x"), ops._ld(x), x.device
        logits = torch.empty(P, self._desc.n_classes, dtype=torch.float32, device=dev)
        ws = self._ws
        if self._desc_h is not None:
            rc = lib.yolat_forward_eval_bf16_loc(ctypes.byref(self._desc_h), xp, ldx, None, 0, 0, None, None, ctypes.byref(gc),
                                                 N, E, P, logits.data_ptr(), logits.stride(0), ws.data_ptr(), ws.numel(),
                                                 self._status.data_ptr(), ctypes.byref(loc) if loc is not None else None, 0,
                                                 ops._stream())
            if rc != 0:
                check(rc, "yolat_forward_eval_bf16_loc")
        else:
            rc = lib.yolat_forward_eval_csr(ctypes.byref(self._desc), xp, ldx, ctypes.byref(gc), N, E, P,
                                            logits.data_ptr(), logits.stride(0), ws.data_ptr(), ws.numel(), ops._stream())
            if rc != 0:
                check(rc, "yolat_forward_eval_csr")
        return logits

    def _launch(self, x, edge, e_attr, bbox_idx, N, E, P, se, sc, loc=None):
        capturing = torch.cuda.is_current_stream_capturing()
        if loc is None and not capturing and self._desc_h is not None:
            loc = self.locality(edge, bbox_idx, N, E, P, se, sc)
        return self._launch_coo(ops._f(x, "x"), ops._ld(x), ops._i(edge, torch.int64, "edge"), se, sc,
                                ops._f(e_attr, "e_attr"), ops._i(bbox_idx, torch.int64, "bbox_idx"), N, E, P, x.device, loc,
                                capturing)

    def _launch_coo(self, xp, ldx, ep, se, sc, ap, bp, N, E, P, dev, loc, capturing):
        """The forward on a COO batch given by addresses.  The workspace is this plan's own: when its previous use was a
        forward of the same shape on the same stream, the CSR-build counters are already zero (the `primed` forms: no
        memset launch).  A hipGraph capture always records the self-contained form (a replay may follow a forward of any
        other shape), and a vouched bf16 forward does not touch the counters: neither uses nor keeps the promise."""
        logits = torch.empty(P, self._desc.n_classes, dtype=torch.float32, device=dev)
        stream = ops._stream()
        ws, h = self._ws, self._desc_h
        key = (ws.data_ptr(), self._desc_key, N, E, P, stream)
        keeps = not capturing and not (h is not None and self._vouched(loc, P))
        primed = PRIMED_WS and keeps and self._primed == key
        self._primed = None
        if h is not None:
            what = "yolat_forward_eval_bf16_loc"
            rc = lib.yolat_forward_eval_bf16_loc(ctypes.byref(h), xp, ldx, ep, se, sc, ap, bp, None, N, E, P,
                                                 logits.data_ptr(), logits.stride(0), ws.data_ptr(), ws.numel(),
                                                 self._status.data_ptr(), ctypes.byref(loc) if loc is not None else None,
                                                 1 if primed else 0, stream)
        else:
            what = "yolat_forward_eval"
            fn = lib.yolat_forward_eval_primed if primed else lib.yolat_forward_eval
            rc = fn(ctypes.byref(self._desc), xp, ldx, ep, se, sc, ap, bp, N, E, P, logits.data_ptr(), logits.stride(0),
                    ws.data_ptr(), ws.numel(), self._status.data_ptr(), stream)
        if rc != 0:
            check(rc, what)
        if keeps:
            self._primed = key
        return logits

    def _run_graph(self, x, edge, e_attr, bbox_idx, N, E, P, se, sc):
        """hipGraph replay of the whole forward (memset + 12 launches -> one graph launch: host enqueue
        ~60 -> ~25 us).  A graph bakes in its input addresses, so it is keyed by them: the FIRST call with a
        given set of input buffers launches directly and only marks the key, the second captures, later ones
        replay.  Callers that stage every batch into the same device buffers (a serving loop, bench.py) hit
        the replay path; one-off inputs (predict's sub-batches) never pay a capture.  The result is copied
        out of the graph's static output, so the returned tensor is owned by the caller as usual."""
        if lib.yolat_profile_enabled():
            return None
        gkey = (x.data_ptr(), edge.data_ptr(), e_attr.data_ptr(), bbox_idx.data_ptr(), ops._ld(x), se, sc, N, E, P)
        ent = self._graphs.get(gkey)
        if ent is None:
            if len(self._graphs) >= 8:
                self._graphs.pop(next(iter(self._graphs)))
            self._graphs[gkey] = False                      # seen once: capture next time
            return None
        if ent is False:
            torch.cuda.current_stream().synchronize()
            g = torch.cuda.CUDAGraph()
            cur = torch.cuda.current_stream()
            # capture on the caller's stream when it is a side stream (torch refuses the default stream)
            ctx = torch.cuda.graph(g) if cur == torch.cuda.default_stream() else torch.cuda.graph(g, stream=cur)
            with ctx:
                static_out = self._launch(x, edge, e_attr, bbox_idx, N, E, P, se, sc)
            ent = self._graphs[gkey] = (g, static_out, (x, edge, e_attr, bbox_idx))   # keep the inputs alive
        g, static_out, _ = ent
        self._primed = None        # the next direct launch must not assume which shape used the workspace last
        g.replay()
        return static_out.clone()

    def check_status(self):
        """Raises on the input-validity flags of the forwards since the last check.  The word belongs to the plan and the
        kernels only ever OR into it: a raised condition is cleared here, so one malformed batch does not condemn every later
        forward of the model."""
        try:
            return ops.check_status_word(self._status)
        except (IndexError, ValueError):
            self._status.zero_()
            raise
