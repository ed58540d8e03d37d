"""yolat_vectorgraphicsrecognition_amd — MI355X (gfx950) native implementation of the YOLaT GNN
message-passing hot path (SparseCADGCN forward / train step over Bezier-curve graphs).

Layout
    csrc/            hand-written HIP kernels + the C ABI (include/yolat_hip.h) -> libyolat_hip.so
    _lib.py          ctypes binding (fails loudly when the library is missing: no CPU fallback)
    ops.py           tensor-level wrappers of the C ABI
    engine.py        hand-scheduled forward / backward of the model blocks
    nn_modules.py    gcn_lib.sparse mirror: MultiSeq, MLP, GraphConv, ResBlock
    architecture.py  cad_recognition/architecture3cc_rpn_gp_iter2 mirror: SparseCADGCN, ...
    submit.py        predict in one submission, detect_submit / evaluate_submit and their handles (behind SparseCADGCN's methods)
    trainer.py       flat-buffer Adam + data-parallel step (RCCL all-reduce of one gradient bucket)
    data.py          Data bag, collate / offset fix-up, synthetic Bezier-graph generators
    augment.py       training augmentation (graph_dict3.random_transfer + update_bbox) on host items / device batches
    proposals.py     box-proposal generation (graph_dict3._get_proposal) over the native window / edge pick-up op
    dropin/          import shims so the reference's own scripts resolve gcn_lib / torch_scatter / ...
"""
from . import _lib  # noqa: F401  (raises if libyolat_hip.so is missing)
from . import ops, engine  # noqa: F401
from .nn_modules import MultiSeq, MLP, GraphConv, ResBlock, scatter  # noqa: F401
from .architecture import Backbone, SparseCADGCN, DetectionLoss, Opt  # noqa: F401
from .data import (Data, DeviceLoader, collate, collate_to_device, item_csr, fixup_offsets, synth_graph, synth_batch, synth_roots, idxTree, config,  # noqa: F401
                   select_tree_nodes, build_subset)
from .postprocess import (non_max_suppression, get_batch_statistics, ap_per_class, compute_ap, bbox_iou,  # noqa: F401
                          non_max_suppression_batched, get_batch_statistics_batched)
from .evaluation import evaluate_batch, detect_batch, detect_batch_async, detect_stream, test as evaluate  # noqa: F401
from .evaluation import evaluate_batch_async, evaluate_stream, confusion_counts, EpochMetrics  # noqa: F401
from .submit import DetectHandle, EvalHandle  # noqa: F401
from .trainer import (FlatParams, FlatAdam, Trainer, shard_graph_ids, allreduce_mean_, broadcast_parameters,  # noqa: F401
                      load_reference_checkpoint)

from .proposals import get_proposal, proposal_windows  # noqa: F401
from . import augment  # noqa: F401
from .augment import AugParams, draw_params, augment_item, augment_batch_  # noqa: F401

__version__ = "0.2.0"
