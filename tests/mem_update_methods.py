"""TEST INFRASTRUCTURE ONLY -- bare objects of the nine tracker classes for their whole `update_memory`: `cls.__new__(cls)` with exactly the
attributes the method reads, small memories (3 slots, one initial sample: from the third of the five calls on the full-memory arg-min runs), seeded
arguments.
tools/make_golden_mem_update.py runs the UNMODIFIED methods on them on the CPU (tests/golden/mem_update_methods.npz); the tests run the
drop-ins of pytracking_amd.memory_update on the same objects on the device.  Needs the reference importable (oracle.ref_harness)."""
import importlib
from types import SimpleNamespace

import numpy as np
import torch

CLASSES = ("DiMP", "KYS", "ToMP", "DiMPSimple", "TaMOs", "KeepTrack", "ATOM", "LWL", "RTS")
MODULES = {"DiMP": "dimp.dimp", "KYS": "kys.kys", "ToMP": "tomp.tomp", "DiMPSimple": "dimp_simple.dimp_simple", "TaMOs": "tamos.tamos",
           "KeepTrack": "keep_track.keep_track", "ATOM": "atom.atom", "LWL": "lwl.lwl", "RTS": "rts.rts"}
N, INIT, CALLS = 3, 1, 5
FEAT = (2, 3, 3)                                   # one sample of the feature memory
LRS = (None, 0.2, None, None, 0.3)
MEMORIES = {"DiMP": ("training_samples", "target_boxes"), "KYS": ("training_samples", "target_boxes"),
            "ToMP": ("training_samples", "target_labels", "target_boxes"), "DiMPSimple": ("training_samples", "target_labels", "target_boxes"),
            "TaMOs": ("training_samples", "target_labels", "target_boxes"),
            "KeepTrack": ("training_samples", "target_labels", "target_boxes", "target_label_certainties", "mem_sort_indices"),
            "ATOM": ("training_samples", "y", "hinge_mask"), "LWL": ("training_samples", "target_masks"), "RTS": ("training_samples", "target_masks")}


def cls_of(name):
    return getattr(importlib.import_module("pytracking.tracker." + MODULES[name]), name)


def _rand(rng, *shape):
    return torch.from_numpy(rng.standard_normal(shape).astype(np.float32))


def bare(name, device="cpu"):
    from pytracking import TensorList
    from pytracking.utils import TrackerParams
    rng = np.random.default_rng(300 + CLASSES.index(name))
    t = cls_of(name).__new__(cls_of(name))
    p = TrackerParams()
    p.learning_rate, p.init_samples_minimum_weight, p.sample_memory_size, p.device = 0.1, 0.25, N, device
    t.params = p
    blocks = 2 if name == "ATOM" else 1
    feats = [FEAT, (3, 2, 2)][:blocks]

    def memory(*shape):
        m = torch.zeros(N, *shape)
        m[:INIT] = _rand(rng, INIT, *shape)
        return m.to(device)
    sw = torch.zeros(N)
    sw[:INIT] = 1.0 / INIT
    t.sample_weights = TensorList([sw.clone().to(device) for _ in range(blocks)])
    t.previous_replace_ind = [None] * blocks
    t.num_init_samples = TensorList([INIT] * blocks)
    t.num_stored_samples = TensorList([INIT] * blocks) if name not in ("LWL", "RTS") else [INIT] * blocks
    t.training_samples = TensorList([memory(*f) for f in feats])
    if name in ("DiMP", "KYS", "ToMP", "DiMPSimple", "KeepTrack"):
        t.target_boxes = memory(4)
    if name in ("ToMP", "DiMPSimple", "KeepTrack"):
        t.target_labels = TensorList([memory(1, 3, 3)])
    if name == "TaMOs":
        t.target_labels, t.target_boxes = TensorList([memory(2, 3, 3)]), memory(2, 4)
    if name == "KeepTrack":
        t.target_label_certainties = torch.zeros(N, 1, 1, 1)
        t.target_label_certainties[:INIT] = 1.0
        t.target_label_certainties = t.target_label_certainties.to(device)
        t.mem_sort_indices, t.candidate_collection = torch.arange(0, INIT), None
    if name == "ATOM":
        t.fparams = [SimpleNamespace(learning_rate=0.1, init_samples_minimum_weight=0.25), SimpleNamespace(learning_rate=0.05)]
        t.y = TensorList([memory(1, f[1], f[2]) for f in feats])
        t.hinge_mask = TensorList([memory(1, f[1], f[2]) for f in feats])
        p.hinge_threshold = 0.05
    if name in ("LWL", "RTS"):
        t.target_masks, p.lower_init_weight = memory(1, 6, 6), True
    return t


def arguments(name, k, device="cpu"):
    """the arguments of call k of `update_memory`, as the tracker's frame loop passes them (boxes and ToMP's label come from the CPU)"""
    from pytracking import TensorList
    rng = np.random.default_rng(900 + 10 * CLASSES.index(name) + k)
    lr = LRS[k]
    x = TensorList([_rand(rng, 3, *FEAT).to(device)[1:2]])                                # test_x[scale_ind:scale_ind+1]
    box = _rand(rng, 4)
    if name in ("DiMP", "KYS"):
        return (x, box, lr)
    if name in ("ToMP", "DiMPSimple"):
        return (x, _rand(rng, 1, 3, 3).to(device), box, lr)
    if name == "TaMOs":
        return (x, {1: TensorList([_rand(rng, 1, 1, 3, 3).to(device)]), 2: TensorList([_rand(rng, 1, 1, 3, 3).to(device)])},
                {1: _rand(rng, 4).to(device), 2: _rand(rng, 4).to(device)}, lr)
    if name == "KeepTrack":
        c = torch.tensor(float(rng.uniform(0.05, 0.9)) if k != 2 else 1e-6)
        return (x, TensorList([_rand(rng, 1, 1, 3, 3).to(device)]), box, lr, c.to(device))
    if name == "ATOM":
        x2 = TensorList([x[0], _rand(rng, 1, 3, 2, 2).to(device)])
        return (x2, TensorList([_rand(rng, 1, 1, 3, 3).to(device), _rand(rng, 1, 1, 2, 2).to(device)]), lr)
    return (x, _rand(rng, 1, 1, 6, 6).to(device), lr)


def snapshot(t, name):
    """every memory, weight, counter and index of the object as numpy"""
    out = {}
    for b, w in enumerate(t.sample_weights):
        out[f"sample_weights.{b}"] = w.detach().cpu().numpy().copy()
    for attr in MEMORIES[name]:
        m = getattr(t, attr)
        for b, v in enumerate(m if isinstance(m, (list, tuple)) else [m]):
            out[f"{attr}.{b}"] = v.detach().cpu().numpy().copy()
    out["previous_replace_ind"] = np.array([-1 if v is None else int(v) for v in t.previous_replace_ind])
    out["num_stored_samples"] = np.array([int(v) for v in t.num_stored_samples])
    return out


def reference_goldens():
    """{"<Class>.<call>.<what>": array}: the state behind every call of the unmodified method, fp32 on the CPU"""
    g = {}
    for name in CLASSES:
        t = bare(name)
        for k in range(CALLS):
            vars(cls_of(name))["update_memory"](t, *arguments(name, k))
            g.update({f"{name}.{k}.{key}": v for key, v in snapshot(t, name).items()})
    return g


def stored(name, args):
    """what call `args` stores, restated per class: [(memory attribute, entry of the list, block whose index chooses the slot, values, op, arg)]
    (op / arg: tests/mem_update_np.py)"""
    import mem_update_np as RN
    f = lambda t: t.detach().cpu().numpy().astype(np.float32).reshape(-1)
    out = [("training_samples", b, b, f(x), RN.COPY, 0.0) for b, x in enumerate(args[0])]
    if name in ("DiMP", "KYS"):
        out.append(("target_boxes", 0, 0, f(args[1]), RN.COPY, 0.0))
    elif name in ("ToMP", "DiMPSimple", "KeepTrack"):
        out += [("target_labels", 0, 0, f(args[1][0]), RN.COPY, 0.0), ("target_boxes", 0, 0, f(args[2]), RN.COPY, 0.0)]
        if name == "KeepTrack":
            c = np.float32(args[4].item())
            out.append(("target_label_certainties", 0, 0, np.array([max(c, np.sqrt(c))], np.float32), RN.COPY, 0.0))
    elif name == "TaMOs":
        out += [("target_labels", 0, 0, np.concatenate([f(args[1][o][0]) for o in (1, 2)]), RN.COPY, 0.0),
                ("target_boxes", 0, 0, np.concatenate([f(args[2][o]) for o in (1, 2)]), RN.COPY, 0.0)]
    elif name == "ATOM":
        for b, y in enumerate(args[1]):
            out += [("y", b, b, f(y), RN.COPY, 0.0), ("hinge_mask", b, b, f(y), RN.THRESH, 0.05)]
    else:
        out.append(("target_masks", 0, 0, f(args[1][0]), RN.COPY, 0.0))
    return out


def block_of(name, t, b, lr_arg):
    """the restatement's block (tests/mem_update_np.py) of entry b of the object's `sample_weights`"""
    rule = {"ATOM": "B", "LWL": "C", "RTS": "C", "KeepTrack": "D"}.get(name, "A")
    lr = lr_arg if lr_arg is not None else (t.fparams[b].learning_rate if name == "ATOM" else t.params.learning_rate)
    floor = getattr(t.fparams[b], "init_samples_minimum_weight", 0.0) if name == "ATOM" else t.params.get("init_samples_minimum_weight", 0.0)
    return dict(weights=t.sample_weights[b].detach().cpu().numpy(), certainty=t.target_label_certainties.detach().cpu().numpy().reshape(-1) if rule == "D" else None,
                num_init=int(t.num_init_samples[b]), num_stored=int(t.num_stored_samples[b]), prev_ind=t.previous_replace_ind[b], rule=rule,
                lower_init_weight=bool(t.params.get("lower_init_weight", False)), lr=lr, floor=floor or 0.0)
