"""Training augmentation: ``SESYDFloorPlan.random_transfer`` (Datasets/graph_dict3.py:283-298, with ``__transform__``
:236-258 and ``__transform_bbox__`` :260-281) and the ``update_bbox`` that ``__getitem__`` runs after it (:934-959) — what
``--data_aug true`` of the reference's training commands switches on.

The augmentation changes no index: ``pos``, the position columns of ``x`` (``feats = [0,0,0,pos]``, :966-969), ``bbox``,
``gt_bbox`` and ``bbox_targets`` move; edges, ``e_attr``, ``bbox_idx`` and labels stay.  So the dataset items stay immutable
(their cached CSR / descriptors / locality records with them) and the batch is augmented AFTER the hand-over, on the
device, by one launch (csrc/augment.hip):

    params = draw_params(len(items))                       # the reference's draws, in its order
    batch, slices = collate_to_device(items, csr=True)
    augment_batch_(batch, slices, params)                  # or: DeviceLoader(..., augment=True)

``augment_item`` is the same arithmetic in numpy on one host item.

Numerics.  Every coordinate is computed in float64 in the reference's operation order — subtract the centre, flip,
rotate, add the centre, add the translation, scale — with every product and sum rounded on its own, and rounded once to
fp32.  Host and device paths give the same bits.  Against the reference's float64 result (whose ``np.matmul`` may fuse a
multiply-add) the fp32 value is equal or adjacent.

The flips are the reference's: ``__transform__`` draws its two flips on EVERY call, so ``pos``, each of the four corners
of ``gt_bbox`` and each of the four corners of ``bbox_targets`` get flips of their own (18 draws per item).  That is a
quirk of the reference; parity is against it.
"""
import random as _py_random_module

import numpy as np
import torch

SCALE_RATIO = 0.6          # graph_dict3.py:284
TRANSLATE_RATIO = 0.1      # graph_dict3.py:288
N_FLIPS = 18               # 2 (pos) + 4 corners x 2 (gt_bbox) + 4 corners x 2 (bbox_targets)
POS_COLS = (3, 4)          # feats = [0, 0, 0, pos]  (graph_dict3.py:966-969)


class AugParams(object):
    """The draws of ``random_transfer`` for B graphs: ``scale`` [B], ``angle`` [B], ``translate`` [B, 2] (float64) and
    ``flips`` [B, 18] (bool) in drawing order: [0:2] flip x / flip y of ``pos``; [2:10] the four corners p0..p3 of
    ``gt_bbox`` (x, y each); [10:18] the four corners of ``bbox_targets``."""

    __slots__ = ("scale", "angle", "translate", "flips")

    def __init__(self, scale, angle, translate, flips):
        self.scale = np.asarray(scale, dtype=np.float64).reshape(-1)
        B = self.scale.shape[0]
        self.angle = np.asarray(angle, dtype=np.float64).reshape(B)
        self.translate = np.asarray(translate, dtype=np.float64).reshape(B, 2)
        self.flips = np.asarray(flips, dtype=bool).reshape(B, N_FLIPS)

    def __len__(self):
        return self.scale.shape[0]

    def __getitem__(self, i):
        """The parameters of graph i (or of a slice of graphs) as an AugParams of their own."""
        if isinstance(i, (int, np.integer)):
            if not -len(self) <= i < len(self):
                raise IndexError(i)
            i = int(i) % len(self)
            i = slice(i, i + 1)
        return AugParams(self.scale[i], self.angle[i], self.translate[i], self.flips[i])

    @classmethod
    def cat(cls, parts):
        """The parameters of several draws back to back (batch order)."""
        parts = list(parts)
        return cls(np.concatenate([p.scale for p in parts]), np.concatenate([p.angle for p in parts]),
                   np.concatenate([p.translate for p in parts]), np.concatenate([p.flips for p in parts]))

    @classmethod
    def identity(cls, B):
        """scale 1, angle 0, no translation, no flips"""
        return cls(np.ones(B), np.zeros(B), np.zeros((B, 2)), np.zeros((B, N_FLIPS), dtype=bool))

    def block(self, flip_at=0):
        """[B, 8] float64 rows ``cos, sin, scale, tx, ty, flip x, flip y, 0`` — the parameter block of
        ``yolat_augment_batch``; ``flip_at``: which pair of ``flips`` (0: the one of ``pos``)."""
        B = len(self)
        out = np.zeros((B, 8), dtype=np.float64)
        out[:, 0] = np.cos(self.angle)
        out[:, 1] = np.sin(self.angle)
        out[:, 2] = self.scale
        out[:, 3:5] = self.translate
        out[:, 5:7] = self.flips[:, flip_at:flip_at + 2]
        return out


def draw_params(B, np_random=None, py_random=None):
    """The draws of B consecutive ``random_transfer`` calls, graph by graph, in the reference's order: four
    ``np.random.random()`` (scale, angle, translate x, translate y; :285-291), then 18 ``random.choice([True, False])``
    (:250-253 through :293-296).  By default the GLOBAL ``numpy.random`` / ``random`` generators, so that under the same
    seeds the parameters are the reference's and both generators are left where the reference leaves them; a
    ``numpy.random.RandomState`` / ``random.Random`` instance each for streams of one's own (per rank, per worker)."""
    npr = np.random if np_random is None else np_random
    pyr = _py_random_module if py_random is None else py_random
    nrand = getattr(npr, "random", None) or npr.random_sample
    B = int(B)
    scale, angle = np.empty(B), np.empty(B)
    translate, flips = np.empty((B, 2)), np.empty((B, N_FLIPS), dtype=bool)
    for b in range(B):
        scale[b] = (nrand() * 2 - 1) * SCALE_RATIO + 1
        angle[b] = nrand() * np.pi * 2
        translate[b, 0] = (nrand() * 2 - 1) * TRANSLATE_RATIO
        translate[b, 1] = (nrand() * 2 - 1) * TRANSLATE_RATIO
        for k in range(N_FLIPS):
            flips[b, k] = pyr.choice([True, False])
    return AugParams(scale, angle, translate, flips)


# ---------------------------------------------------------------------------------------------
# host path (numpy).  The same operations, in the same order, as k_augment_batch.
# ---------------------------------------------------------------------------------------------

def _transform_points(px, py, row, fx, fy):
    """__transform__ (:236-258) on float64 coordinate arrays, element-wise; row = one row of AugParams.block()."""
    c, s, scale, tx, ty = (np.float64(v) for v in row[:5])
    px = px - 0.5
    py = py - 0.5
    if fx:
        px = -px
    if fy:
        py = -py
    ns = -s
    rx = px * c + py * ns                       # numpy rounds the products and the sum one by one (no fma)
    ry = px * s + py * c
    rx = rx + 0.5
    ry = ry + 0.5
    rx = rx + tx
    ry = ry + ty
    ox = rx * scale + ry * 0.0                  # pos @ diag(scale): the zero products are the reference's
    oy = rx * 0.0 + ry * scale
    return ox, oy


def _transform_boxes(box, row, flips8):
    """__transform_bbox__ (:260-281): the four corners p0 = (x0, y0), p1 = (x1, y0), p2 = (x1, y1), p3 = (x0, y1), each
    through __transform__ with flips of ITS OWN, then the bounding rectangle.  box [n, 4] float64 -> [n, 4] float64."""
    x0, y0, x1, y1 = box[:, 0], box[:, 1], box[:, 2], box[:, 3]
    xs, ys = [], []
    for k, (cx, cy) in enumerate(((x0, y0), (x1, y0), (x1, y1), (x0, y1))):
        ox, oy = _transform_points(cx, cy, row, bool(flips8[2 * k]), bool(flips8[2 * k + 1]))
        xs.append(ox)
        ys.append(oy)
    xs, ys = np.stack(xs, 1), np.stack(ys, 1)
    if xs.shape[0] == 0:
        return np.zeros((0, 4), dtype=np.float64)
    return np.stack([xs.min(1), ys.min(1), xs.max(1), ys.max(1)], 1)


def _as_f64(t):
    return t.detach().cpu().numpy().astype(np.float64)


def _boxes_of(pos32, bbox_idx, old_bbox):
    """update_bbox (:934-959) over a SORTED bbox_idx with the row count of old_bbox: row p = (min x, min y, max x, max y)
    of the nodes with bbox_idx == p; a proposal without a node keeps its old row."""
    P = old_bbox.shape[0]
    out = old_bbox.copy()
    if P == 0 or pos32.shape[0] == 0:
        return out
    seg = np.searchsorted(bbox_idx, np.arange(P + 1))
    has = seg[1:] > seg[:-1]
    starts = seg[:-1][has]
    out[has, 0:2] = np.minimum.reduceat(pos32, starts, axis=0)
    out[has, 2:4] = np.maximum.reduceat(pos32, starts, axis=0)
    return out


# what a new item may inherit from the caches on the old one: they depend on the index tensors (shared) and row counts only
_KEEP_CACHES = ("_yolat_csr", "_yolat_loc_item", "_yolat_keysplit")


def augment_item(item, params, cols=POS_COLS):
    """``random_transfer`` + ``update_bbox`` on ONE host item with the draws ``params`` (an AugParams of one graph:
    ``draw_params(1)`` or ``draw_params(B)[i]``).  Returns a NEW item: ``pos``, ``x[:, cols]``, ``bbox`` — and
    ``gt_bbox`` / ``bbox_targets`` when the item has them — are new fp32 tensors, every other attribute is shared with
    ``item``, which is not touched.  The new item keeps the cached CSR and locality record (functions of the shared index tensors) and
    drops the cached collate descriptors (they hold addresses of the replaced tensors)."""
    if len(params) != 1:
        raise ValueError("augment_item takes the parameters of one graph (params[i]), got %d" % len(params))
    row = params.block()[0]
    fl = params.flips[0]
    d = item.__dict__
    new = item.__class__()
    nd = new.__dict__
    for k, v in d.items():
        if k[0] != "_" or k in _KEEP_CACHES:
            nd[k] = v
    pos = _as_f64(item.pos)
    ox, oy = _transform_points(pos[:, 0], pos[:, 1], row, bool(fl[0]), bool(fl[1]))
    pos32 = np.stack([ox, oy], 1).astype(np.float32)            # the one rounding
    nd["pos"] = torch.from_numpy(pos32)
    x = item.x.clone()
    x[:, cols[0]] = nd["pos"][:, 0].to(x.dtype)
    x[:, cols[1]] = nd["pos"][:, 1].to(x.dtype)
    nd["x"] = x
    bidx = item.bbox_idx.numpy()
    if bidx.shape[0] > 1 and np.any(bidx[1:] < bidx[:-1]):
        raise ValueError("bbox_idx is not non-decreasing")
    nd["bbox"] = torch.from_numpy(_boxes_of(pos32, bidx, item.bbox.detach().cpu().numpy().astype(np.float32)))
    for key, at in (("gt_bbox", 2), ("bbox_targets", 10)):
        t = d.get(key)
        if t is not None:
            nd[key] = torch.from_numpy(_transform_boxes(_as_f64(t).reshape(-1, 4), row, fl[at:at + 8])
                                       .astype(np.float32)).reshape(t.shape)
    return new


# ---------------------------------------------------------------------------------------------
# device path
# ---------------------------------------------------------------------------------------------

def augment_batch_(batch, slices, params, stream=None, cols=POS_COLS):
    """``random_transfer`` + ``update_bbox`` IN PLACE on a device batch of ``collate_to_device`` (either ``csr`` mode) or
    of a ``DeviceLoader``: one small H2D copy (the parameter block and the per-graph proposal offsets, from pinned
    memory) and one launch (``yolat_augment_batch``) on ``stream`` (a ``torch.cuda.Stream``; default: the current one),
    nothing read back.  ``params``: the draws of the batch's graphs, in batch order.  ``batch.pos``, the position
    columns of ``batch.x`` and ``batch.bbox`` change on the device; ``gt_bbox`` / ``bbox_targets``, which stay on the host
    in a collated batch, are replaced there by transformed copies (per-graph ranges from their own ``slices`` entries).
    A proposal without a node keeps its ``bbox`` row.  Returns ``batch``."""
    from . import ops
    if stream is not None:
        with torch.cuda.stream(stream):
            return augment_batch_(batch, slices, params, None, cols)
    prop = slices["labels"] if "labels" in slices else slices["bbox"]
    B = int(prop.shape[0]) - 1
    if len(params) != B:
        raise ValueError("augment_batch_: %d parameter rows for a batch of %d graphs" % (len(params), B))
    pos, x, bbox = batch.pos, batch.x, batch.bbox
    if B > 0 and pos.shape[0] > 0 and bbox.shape[0] > 0:
        g = batch.__dict__.get("_yolat_graph")
        if g is not None:
            seg_ptr = g.seg_ptr
        else:
            seg_ptr = ops.segment_ptr(batch.bbox_idx, bbox.shape[0])
        # parameter block [B, 8] float64 and prop_ptr [B + 1] int64 side by side: one pinned buffer, one copy
        stage = torch.empty(9 * B + 1, dtype=torch.float64, pin_memory=True)
        stage[:8 * B].view(B, 8).numpy()[...] = params.block()
        stage[8 * B:].view(torch.int64).copy_(prop.to(torch.int64))
        dev = stage.to(pos.device, non_blocking=True)
        ops.augment_batch(pos, x, seg_ptr, dev[8 * B:].view(torch.int64), bbox, dev[:8 * B].view(B, 8), cols)
    for key, at in (("gt_bbox", 2), ("bbox_targets", 10)):
        t = getattr(batch, key, None)
        if t is None:
            continue
        if not isinstance(t, torch.Tensor) or t.is_cuda:
            raise TypeError("augment_batch_: %s must be a host tensor (collate keeps it there)" % key)
        s = slices[key]
        if int(s.shape[0]) - 1 != B:
            raise ValueError("augment_batch_: slices[%r] does not describe %d graphs" % (key, B))
        blk = params.block()
        # a NEW tensor: the collate of a one-item batch hands the item's own tensor through
        v = t.reshape(-1, 4).to(torch.float32).clone()
        for b in range(B):
            lo, hi = int(s[b]), int(s[b + 1])
            if hi > lo:
                out = _transform_boxes(v[lo:hi].numpy().astype(np.float64), blk[b], params.flips[b, at:at + 8])
                v[lo:hi] = torch.from_numpy(out.astype(np.float32))
        setattr(batch, key, v.reshape(t.shape))
    return batch
