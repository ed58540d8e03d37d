"""GPU tests of the training augmentation (csrc/augment.hip through augment.augment_batch_ / DeviceLoader(augment=...)):
against tests/golden/augment.npz (the reference's own random_transfer + update_bbox), against the numpy host path
augment.augment_item bit for bit, at edge layouts, and end to end through the eval forward and one training step."""
import os
import random

import numpy as np
import pytest
import torch

import augment_util as au
import golden_util as gu

pytestmark = pytest.mark.gpu


def _yv():
    import yolat_vectorgraphicsrecognition_amd as yv
    return yv


def _seed(s):
    np.random.seed(s)
    random.seed(s)


def _shape_items(yv, shape):
    """host items of a batch shaped like cfg 3 (4 x 2000 proposals of 4 - 40 nodes) / cfg 4 (32 x 300 proposals of 4 - 24)"""
    if shape == "cfg3":
        return [yv.synth_graph(num_proposals=2000, nodes_lo=4, nodes_hi=40, edge_factor=1.2, seed=3000 + i, augmented=True)
                for i in range(4)]
    return [yv.synth_graph(num_proposals=300, nodes_lo=4, nodes_hi=24, edge_factor=1.2, n_classes=22, seed=4000 + i,
                           augmented=True) for i in range(32)]


def _device_batch(yv, items, source, params=None):
    """(batch, slices, loader-or-None) from collate_to_device(csr=True / False) or a DeviceLoader; `params`: let the loader
    augment with exactly these draws"""
    if source == "csr":
        return yv.collate_to_device(items, csr=True) + (None,)
    if source == "coo":
        return yv.collate_to_device(items, csr=False) + (None,)
    loader = yv.DeviceLoader([items], slots=2, csr=(source == "loader"),
                             augment=None if params is None else (lambda B: params))
    batch, slices = next(loader)
    return batch, slices, loader


def _graph_arrays(batch):
    g = batch.__dict__.get("_yolat_graph")
    if g is None:
        return {k: batch[k].clone() for k in ("edge", "e_attr", "bbox_idx")}
    return {k: getattr(g, k).clone() for k in ("row_ptr", "src", "dst", "attr", "seg_ptr", "node_seg")}


def _host_want(yv, items, params):
    new = [yv.augment_item(it, params[i]) for i, it in enumerate(items)]
    return new, {k: torch.cat([n[k] for n in new], 0) for k in ("pos", "x", "bbox")}


@pytest.fixture(scope="module")
def fixture(golden_dir):
    return np.load(os.path.join(golden_dir, "augment.npz"))


@pytest.mark.parametrize("source", ["csr", "coo", "loader"])
def test_device_path_meets_the_contract_on_the_reference_fixture(fixture, source):
    """The three fixture items as ONE batch; graph i gets the draws the reference made for (case i, seed) — each case was
    recorded under a seeding of its own.  pos / bbox come back from the device, gt_bbox / bbox_targets from the host side
    of the batch, all four against float32(reference float64): the bound for every element, the cap on the share of
    elements that are not bit-identical."""
    yv = _yv()
    c = au.Contract()
    names = list(au.CASES)
    items = [au.item_from_inputs(au.fixture_case(fixture, n), yv.Data, seed=i) for i, n in enumerate(names)]
    for s in au.SEEDS:
        parts = []
        for n in names:
            _seed(s)
            parts.append(yv.draw_params(1))
        params = yv.AugParams.cat(parts)
        batch, slices, loader = _device_batch(yv, items, source)
        yv.augment_batch_(batch, slices, params)
        torch.cuda.synchronize()
        for i, n in enumerate(names):
            for k in ("pos", "bbox", "gt_bbox", "bbox_targets"):
                lo, hi = int(slices[k][i]), int(slices[k][i + 1])
                c.check(batch[k][lo:hi].cpu().numpy(), fixture["%s/s%d/%s" % (n, s, k)], "%s/s%d/%s" % (n, s, k))
        assert torch.equal(batch.x[:, 3:5], batch.pos)
        if loader is not None:
            loader.close()
    c.finish()


@pytest.mark.parametrize("source", ["csr", "coo", "loader"])
@pytest.mark.parametrize("shape", ["cfg3", "cfg4"])
def test_device_path_equals_the_host_path_bit_for_bit(shape, source):
    yv = _yv()
    items = _shape_items(yv, shape)
    _seed(31)
    params = yv.draw_params(len(items))
    _, want = _host_want(yv, items, params)
    batch, slices, loader = _device_batch(yv, items, source)
    before = {"x3": batch.x[:, :3].clone(), "stat_feats": batch.stat_feats.clone(), "labels": batch.labels.clone()}
    g_before = _graph_arrays(batch)
    assert not torch.equal(batch.pos.cpu(), want["pos"])
    yv.augment_batch_(batch, slices, params)
    torch.cuda.synchronize()
    assert torch.equal(batch.pos.cpu(), want["pos"])
    assert torch.equal(batch.x[:, 3:5].cpu(), want["x"][:, 3:5])
    assert torch.equal(batch.bbox.cpu(), want["bbox"])
    assert torch.equal(batch.x[:, :3], before["x3"])
    assert torch.equal(batch.stat_feats, before["stat_feats"]) and torch.equal(batch.labels, before["labels"])
    for k, v in _graph_arrays(batch).items():
        assert torch.equal(v, g_before[k]), k
    if loader is not None:
        loader.close()


@pytest.mark.parametrize("csr", [True, False])
def test_edge_layouts_one_graph_seven_columns_side_stream(csr):
    """B = 1; proposals of 1, 65 and 1500 nodes next to ordinary ones; x with C = 7 (the positions still in columns 3, 4,
    the others untouched); the launch on a stream that is not the current one."""
    yv = _yv()
    inp = au.inputs_of_sizes((1, 65, 7, 1500, 1, 16, 17, 64), seed=5)
    item = au.item_from_inputs(inp, yv.Data, C=7, seed=2)
    params = yv.AugParams([0.55], [4.0], [[-0.09, 0.1]], np.arange(18) % 3 == 0)
    _, want = _host_want(yv, [item], params)
    batch, slices = yv.collate_to_device([item], csr=csr)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    yv.augment_batch_(batch, slices, params, stream=side)
    side.synchronize()
    assert torch.equal(batch.pos.cpu(), want["pos"]) and torch.equal(batch.bbox.cpu(), want["bbox"])
    assert torch.equal(batch.x.cpu(), want["x"]) and batch.x.shape[1] == 7
    assert torch.equal(batch.x[:, [0, 1, 2, 5, 6]].cpu(), item.x[:, [0, 1, 2, 5, 6]])
    # the boxes are what torch makes of the new positions
    idx = item.bbox_idx.cuda()[:, None].expand(-1, 2)
    P = item.bbox.shape[0]
    lo = torch.full((P, 2), float("inf"), device="cuda").scatter_reduce(0, idx, batch.pos, "amin")
    hi = torch.full((P, 2), float("-inf"), device="cuda").scatter_reduce(0, idx, batch.pos, "amax")
    assert torch.equal(batch.bbox, torch.cat([lo, hi], 1))


def test_identity_parameters_return_the_positions_and_the_exact_boxes():
    """scale 1, angle 0, no translation, no flips on positions that are multiples of 2^-24: every float64 step is exact, so
    pos comes back unchanged and bbox is exactly the amin / amax over bbox_idx."""
    yv = _yv()
    items = [yv.synth_graph(num_proposals=40 + 9 * i, nodes_lo=2, nodes_hi=30, seed=70 + i) for i in range(3)]
    rng = np.random.default_rng(12)
    for it in items:
        p = (rng.integers(0, 1 << 24, size=tuple(it.pos.shape)).astype(np.float64) / (1 << 24)).astype(np.float32)
        it.pos = torch.from_numpy(p)
        it.x = it.x.clone()
        it.x[:, 3:5] = it.pos
    batch, slices = yv.collate_to_device(items, csr=False)
    pos0, x0 = batch.pos.clone(), batch.x.clone()
    yv.augment_batch_(batch, slices, yv.AugParams.identity(3))
    torch.cuda.synchronize()
    assert torch.equal(batch.pos, pos0) and torch.equal(batch.x, x0)
    idx = batch.bbox_idx[:, None].expand(-1, 2)
    P = batch.bbox.shape[0]
    lo = torch.full((P, 2), float("inf"), device="cuda").scatter_reduce(0, idx, pos0, "amin")
    hi = torch.full((P, 2), float("-inf"), device="cuda").scatter_reduce(0, idx, pos0, "amax")
    assert torch.equal(batch.bbox, torch.cat([lo, hi], 1))


@pytest.mark.parametrize("csr", [True, False])
def test_loader_with_augment_equals_collate_draw_and_augment_over_several_batches(csr):
    """DeviceLoader(augment=True) under fixed seeds == collate_to_device + draw_params + augment_batch_, batch after batch:
    the loader draws when a batch is drawn, in batch order, from the global generators."""
    yv = _yv()
    lists = [[yv.synth_graph(num_proposals=20 + 11 * ((i + j) % 3), nodes_lo=2, nodes_hi=12 + 5 * j, seed=900 + 10 * i + j)
              for j in range(1 + (i * 2) % 4)] for i in range(6)]
    _seed(123)
    got = []
    loader = yv.DeviceLoader(lists, slots=3, csr=csr, augment=True)
    for batch, slices in loader:
        got.append({k: batch[k].clone() for k in ("pos", "x", "bbox", "stat_feats", "labels")})
        assert len(batch._aug_params) == len(slices["labels"]) - 1
    loader.close()
    end_state = (np.random.random(), random.random())
    assert len(got) == len(lists)
    _seed(123)
    for items, g in zip(lists, got):
        batch, slices = yv.collate_to_device(items, csr=csr)
        yv.augment_batch_(batch, slices, yv.draw_params(len(items)))
        for k, v in g.items():
            assert torch.equal(batch[k], v), k
    assert (np.random.random(), random.random()) == end_state
    # augment=None: the loader's batches are the plain ones
    plain = yv.DeviceLoader(lists[:2], slots=2, csr=csr)
    for (batch, slices), items in zip(plain, lists[:2]):
        wb, _ = yv.collate_to_device(items, csr=csr)
        assert torch.equal(batch.pos, wb.pos) and torch.equal(batch.bbox, wb.bbox) and "_aug_params" not in batch.__dict__
    plain.close()


@pytest.mark.parametrize("csr", [True, False])
def test_a_proposal_without_a_node_keeps_its_bbox_row(csr):
    yv = _yv()
    items = [yv.synth_graph(num_proposals=9, nodes_lo=3, nodes_hi=8, seed=60 + i) for i in range(2)]
    for it in items:
        b = it.bbox_idx.clone()
        b[b == 4] = 5                      # proposal 4 of either item loses its nodes (no edge leaves a proposal)
        it.bbox_idx = b
    _seed(8)
    params = yv.draw_params(2)
    _, want = _host_want(yv, items, params)
    batch, slices = yv.collate_to_device(items, csr=csr)
    old = batch.bbox.clone()
    yv.augment_batch_(batch, slices, params)
    torch.cuda.synchronize()
    assert torch.equal(batch.bbox[4], old[4]) and torch.equal(batch.bbox[13], old[13])
    keep = torch.ones(18, dtype=torch.bool)
    keep[[4, 13]] = False
    assert not torch.equal(batch.bbox[keep.cuda()], old[keep.cuda()])
    assert torch.equal(batch.bbox.cpu(), want["bbox"]) and torch.equal(batch.pos.cpu(), want["pos"])


def test_wrapper_checks_dtype_shape_and_device():
    yv = _yv()
    dev = "cuda"
    pos, x = torch.zeros(6, 2, device=dev), torch.zeros(6, 5, device=dev)
    seg, prop = torch.tensor([0, 3, 6], dtype=torch.int32, device=dev), torch.tensor([0, 2], device=dev)
    bbox, par = torch.zeros(2, 4, device=dev), torch.zeros(1, 8, dtype=torch.float64, device=dev)
    par[0, 0] = par[0, 2] = 1.0
    yv.ops.augment_batch(pos, x, seg, prop, bbox, par)              # the well-formed call
    with pytest.raises(TypeError):
        yv.ops.augment_batch(pos, x, seg, prop, bbox, par.float())
    with pytest.raises(TypeError):
        yv.ops.augment_batch(pos, x, seg.long(), prop, bbox, par)
    with pytest.raises(ValueError):
        yv.ops.augment_batch(pos, x, seg, prop, bbox, par, cols=(3, 5))
    with pytest.raises(ValueError):
        yv.ops.augment_batch(pos, x[:4], seg, prop, bbox, par)
    with pytest.raises(ValueError):
        yv.ops.augment_batch(pos.t().contiguous().t(), x, seg, prop, bbox, par)
    with pytest.raises(RuntimeError):
        yv.ops.augment_batch(pos, x, seg, prop, bbox.cpu(), par)
    batch, slices = yv.collate_to_device([yv.synth_graph(num_proposals=4, nodes_lo=3, nodes_hi=5, seed=1)], csr=True)
    with pytest.raises(ValueError):
        yv.augment_batch_(batch, slices, yv.AugParams.identity(2))
    with pytest.raises(TypeError):
        yv.DeviceLoader([], augment=3)
    torch.cuda.synchronize()


@pytest.mark.parametrize("source", ["csr", "loader", "loader_coo"])
def test_forward_and_training_step_on_a_device_augmented_batch_equal_those_on_host_augmented_items(source):
    """End to end: the eval forward on a device-augmented batch == the forward on a batch collated from augment_item's
    outputs, bit for bit (logits and boxes); one Trainer.step on each gives the same loss bits and parameters."""
    yv = _yv()
    items = [yv.synth_graph(num_proposals=30 + 10 * i, nodes_lo=4, nodes_hi=20, edge_factor=1.3, seed=800 + i)
             for i in range(3)]
    _seed(17)
    params = yv.draw_params(len(items))
    new, _ = _host_want(yv, items, params)
    opt = yv.Opt()
    csr = source != "loader_coo"

    def forward(batch, slices):
        model = gu.fill_state_(yv.SparseCADGCN(opt), 17).cuda().eval()
        with torch.no_grad():
            logits, boxes = model(batch, slices)
        torch.cuda.synchronize()
        return logits.clone(), boxes.clone()

    def step(batch, slices):
        model = gu.fill_state_(yv.SparseCADGCN(opt), 17).cuda()
        tr = yv.Trainer(model, opt, lr=1e-3, weight_decay=1e-5)
        loss = float(tr.step(batch, slices))
        torch.cuda.synchronize()
        return loss, [p.detach().clone() for p in model.parameters()]

    for run in (forward, step):
        if source == "csr":
            batch, slices, loader = _device_batch(yv, items, "csr")
            yv.augment_batch_(batch, slices, params)
        else:
            batch, slices, loader = _device_batch(yv, items, source, params)
        got = run(batch, slices)
        if loader is not None:
            loader.close()
        want = run(*yv.collate_to_device(new, csr=csr))
        if run is forward:
            assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
        else:
            assert got[0] == want[0]
            assert all(torch.equal(a, b) for a, b in zip(got[1], want[1]))
