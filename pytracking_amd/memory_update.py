"""Host-side mirror of the trackers' per-frame sample-memory update (include/pt_mem.h, csrc_mem/mem_update.hip): what `update_memory` ->
`update_sample_weights` do at the end of an update frame in every tracker class of the reference -- decay the sample weights, choose the
slot, renormalise, apply the `init_samples_minimum_weight` floor, store the new sample with its label / box / mask -- in two launches and
at most ONE host wait (none while the memory fills: the index is a host value then).

Two ways in:

`run(blocks, rows)` for callers that own their frame loop: `blocks` are `Block`s (one per entry of `sample_weights`), `rows` are `Row`s (one
per tensor stored into the chosen slot).  Returns the Python ints of `replace_ind`.

`make(name)`: per tracker class the (covered, fast) pair `install(memory=True)` binds in place of `update_memory` (DiMP, KYS, ToMP, DiMPSimple,
TaMOs, KeepTrack, ATOM, LWL, RTS), built from the one table `TABLE`: class, rule, the method's arguments, which attributes become rows.
Each reproduces the rest of the reference method as the reference writes it (`previous_replace_ind`, the `num_stored_samples` statement of
that class, TaMOs's assembly of `sample_y` / `target_box`, KeepTrack's `torch.max(c, sqrt(c))` and `mem_sort_indices` bookkeeping).  Calls
the kernels do not cover -- a tracker on the CPU, memories that are not contiguous float32, sizes outside include/pt_mem.h, a source that
overlaps its memory -- go to the reference method (or raise under `install(strict=True)`).

Not covered, still the reference's Python: `rts/clf_branch.py`'s own memory, `get_label_function` (built on the CPU and uploaded by ToMP /
KeepTrack / DiMPSimple / ATOM), `init_memory` (which still calls the reference's `update_sample_weights*`: those stay bound), and ECO, whose
weights live on the host (install(eco=True)).
"""
import collections
import ctypes
import threading

import torch

from . import _lib_mem as _L
from .filter import device_guarded

COPY, THRESH, SCALAR = _L.PT_MEM_COPY, _L.PT_MEM_THRESH, _L.PT_MEM_SCALAR

# weights (n) device float32, updated in place; certainty (n) or None (rule 'D'); prev_ind None or int; lr, floor Python floats (floor 0: none)
Block = collections.namedtuple("Block", "weights num_init num_stored prev_ind lr floor rule certainty lower_init_weight",
                               defaults=(0.0, "A", None, False))
# dst (n, ...) device float32: the whole memory; src (...) one slot's worth, or None with op SCALAR; block: whose index chooses the slot
Row = collections.namedtuple("Row", "src dst block op arg", defaults=(0, COPY, 0.0))


def _dev(t):
    """the address of a contiguous float32 device tensor (None stays None)"""
    if t is None:
        return None
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
        raise RuntimeError("pytracking_amd ops run on the MI355X only, on contiguous fp32 tensors")
    return t.data_ptr()


def c_block(b):
    q = _L.MemBlock()
    q.weights, q.certainty = _dev(b.weights), _dev(b.certainty)
    q.n, q.num_init, q.num_stored = b.weights.numel(), int(b.num_init), int(b.num_stored)
    q.prev_ind = -1 if b.prev_ind is None else int(b.prev_ind)
    q.rule, q.lower_init_weight = _L.RULES.index(b.rule), int(bool(b.lower_init_weight))
    q.lr, q.floor = float(b.lr), float(b.floor or 0.0)
    return q


def c_row(r):
    q = _L.MemRow()
    q.src, q.dst = _dev(r.src), _dev(r.dst)
    q.elems = r.dst.numel() // r.dst.shape[0]
    if r.src is not None and r.src.numel() != q.elems:
        raise ValueError(f"memory_update: a source of {r.src.numel()} elements for slots of {q.elems}")
    q.block, q.op, q.arg = int(r.block), int(r.op), float(r.arg)
    return q


class MemoryUpdate:
    """Per (device, stream): the pinned result record, its sequence number and the workspace."""

    def __init__(self, device):
        t = torch.zeros(_L.PT_MEM_REC_FLOATS, dtype=torch.float32).pin_memory()
        self.rec, self.host, self.rec_ptr = t, t.numpy(), ctypes.c_void_p(t.data_ptr())
        self.seq = 0.0
        self.ws = torch.empty(512, dtype=torch.uint8, device=device)
        self.ws_ptr = ctypes.c_void_p((self.ws.data_ptr() + 255) // 256 * 256)
        self.waits = 0                                             # calls that waited on the record

    def queue(self, blocks, rows):
        """Queue both launches on the current stream -> the host indices (-1 where the index comes from the device)."""
        B, R = len(blocks), len(rows)
        for r in rows:                                             # the slot index runs over the block's n: the memory has to hold n slots
            if not 0 <= r.block < B or r.dst.shape[0] != blocks[r.block].weights.numel():
                raise ValueError("memory_update: a row whose memory does not have one slot per weight of its block")
        cb, cr = (_L.MemBlock * max(B, 1))(*[c_block(b) for b in blocks]), (_L.MemRow * max(R, 1))(*[c_row(r) for r in rows])
        lib = _L.lib()
        self.seq = self.seq + 1.0 if self.seq < 8388607.0 else 1.0
        rc = lib.pt_mem_update_f32(cb, B, cr if R else None, R, self.rec_ptr, self.seq, self.ws_ptr, 256,
                                   ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        if rc == _L.PT_MEM_ERR_UNSUPPORTED:
            raise NotImplementedError("memory_update: request outside the gfx950 memory update (include/pt_mem.h)")
        _L.check(rc, "pt_mem_update_f32")
        return [lib.pt_mem_host_index(ctypes.byref(cb[b])) for b in range(B)]

    def wait(self):
        """The record of the last queued call, after the one wait: (indices, floor flags, sums) per block slot."""
        _L.check(_L.lib().pt_mem_wait_f32(self.rec_ptr, self.seq, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), "pt_mem_wait_f32")
        self.waits += 1
        v, M = self.host.tolist(), _L.PT_MEM_MAX_BLOCKS
        return ([int(x) for x in v[_L.PT_MEM_R_INDEX:_L.PT_MEM_R_INDEX + M]], [int(x) for x in v[_L.PT_MEM_R_FLOOR:_L.PT_MEM_R_FLOOR + M]],
                v[_L.PT_MEM_R_SUM:_L.PT_MEM_R_SUM + M])

    def run(self, blocks, rows):
        """`replace_ind` as Python ints.  Where pt_mem_host_index answers for every block it does not wait at all."""
        idx = self.queue(blocks, rows)
        if any(i < 0 for i in idx):
            idx = self.wait()[0][:len(blocks)]
        return idx


_CONTEXTS = {}


def context(device=None):
    """The MemoryUpdate of the device's current stream."""
    device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    key = (device.index if device.index is not None else torch.cuda.current_device(), torch.cuda.current_stream(device).cuda_stream)
    if key not in _CONTEXTS:
        _CONTEXTS[key] = MemoryUpdate(device)
    return _CONTEXTS[key]


@device_guarded
def _run(first, blocks, rows):
    return context(first.device).run(blocks, rows)


def run(blocks, rows=()):
    """One memory update on the current stream of the blocks' device -> [replace_ind per block]."""
    return _run(blocks[0].weights, list(blocks), list(rows))


# ---------------------------------------------------------------------------------------------------------------------------------
# drop-ins for `update_memory` of the unmodified tracker classes: the (covered, fast) pairs of install._dispatcher
# ---------------------------------------------------------------------------------------------------------------------------------
LIST, FIRST = "list", "first"       # a row per block, zipped as the reference zips it / one tensor stored at replace_ind[0]
Entry = collections.namedtuple("Entry", "module rule args rows saturate")
# rows: (memory attribute, argument that is stored, LIST or FIRST, op)
_X, _Y, _BOX = ("training_samples", "sample_x", LIST, COPY), ("target_labels", "sample_y", LIST, COPY), ("target_boxes", "target_box", FIRST, COPY)
_MASK = ("target_masks", "mask", FIRST, COPY)
TABLE = collections.OrderedDict([
    ("DiMP", Entry("pytracking.tracker.dimp.dimp", "A", ("sample_x", "target_box", "learning_rate"), (_X, _BOX), False)),
    ("KYS", Entry("pytracking.tracker.kys.kys", "A", ("sample_x", "target_box", "learning_rate"), (_X, _BOX), False)),
    ("ToMP", Entry("pytracking.tracker.tomp.tomp", "A", ("sample_x", "sample_y", "target_box", "learning_rate"), (_X, _Y, _BOX), False)),
    ("DiMPSimple", Entry("pytracking.tracker.dimp_simple.dimp_simple", "A", ("sample_x", "sample_y", "target_box", "learning_rate"), (_X, _Y, _BOX), False)),
    ("TaMOs", Entry("pytracking.tracker.tamos.tamos", "A", ("sample_x", "sample_ys_dict", "target_boxes_dict", "learning_rate"), (_X, _Y, _BOX), False)),
    ("KeepTrack", Entry("pytracking.tracker.keep_track.keep_track", "D",
                        ("sample_x", "sample_y", "target_box", "learning_rate", "target_label_certainty"),
                        (_X, _Y, ("target_label_certainties", "target_label_certainty", FIRST, COPY), _BOX), False)),
    ("ATOM", Entry("pytracking.tracker.atom.atom", "B", ("sample_x", "sample_y", "learning_rate"),
                   (_X, ("y", "sample_y", LIST, COPY), ("hinge_mask", "sample_y", LIST, THRESH)), False)),
    ("LWL", Entry("pytracking.tracker.lwl.lwl", "C", ("sample_x", "mask", "learning_rate"), (_X, _MASK), True)),
    ("RTS", Entry("pytracking.tracker.rts.rts", "C", ("sample_x", "mask", "learning_rate"), (_X, _MASK), True)),
])


def _memory_ok(t):
    return isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.dim() >= 1


def _bind(entry, args, kw):
    names = entry.args
    if len(args) > len(names) or any(k not in names for k in kw):
        return None
    a = dict(zip(names, args))
    if any(k in a for k in kw):
        return None
    a.update(kw)
    for k in names[-2:] if names[-1] == "target_label_certainty" else names[-1:]:
        a.setdefault(k, None)
    return a if all(k in a for k in names) else None


def _blocks(self, entry, a):
    """the `Block`s the reference's zip makes, or None when they are outside the kernels"""
    sw, prev, stored, inits = self.sample_weights, self.previous_replace_ind, self.num_stored_samples, self.num_init_samples
    B = len(sw)
    if not (1 <= B <= _L.PT_MEM_MAX_BLOCKS and len(prev) == len(stored) == len(inits) == B):
        return None
    lr_arg = a["learning_rate"]
    if lr_arg is not None and not isinstance(lr_arg, (int, float)):
        return None
    out = []
    for b in range(B):
        w = sw[b]
        if not (_memory_ok(w) and w.dim() == 1 and w.numel() <= _L.PT_MEM_MAX_WEIGHTS):
            return None
        if entry.rule == "B":
            if len(self.fparams) != B:
                return None
            lr = lr_arg if lr_arg is not None else self.fparams[b].learning_rate
            floor = getattr(self.fparams[b], "init_samples_minimum_weight", None)
        else:
            lr = lr_arg if lr_arg is not None else self.params.learning_rate
            floor = self.params.get("init_samples_minimum_weight", None)
        floor = floor or 0.0
        n, ni, ns = w.numel(), int(inits[b]), int(stored[b])
        if not (isinstance(lr, (int, float)) and 0.0 <= lr <= 1.0 and isinstance(floor, (int, float)) and floor >= 0.0 and 0 <= ni <= n and ns >= 0):
            return None
        if prev[b] is not None and not 0 <= int(prev[b]) < n:
            return None
        cert = None
        if entry.rule == "D":
            cert = self.target_label_certainties
            if b != 0 or not (_memory_ok(cert) and cert.numel() == n and cert.device == w.device):
                return None
        blk = Block(w, ni, ns, prev[b], float(lr), float(floor), entry.rule, cert,
                    bool(self.params.get("lower_init_weight", False)) if entry.rule == "C" else False)
        reset = ns == 0 or lr == 1
        if floor and (ni == 0 or (ni == n and not reset and (entry.rule == "B" or ns >= n))):
            return None                                            # the reference raises there: let it
        out.append(blk)
    return out


def _pairs(self, entry, a):
    """(memory, source, block, op) in the reference's order of statements; None for a statement the rows cannot express"""
    B, out = len(self.sample_weights), []
    for attr, arg, kind, op in entry.rows:
        mem = getattr(self, attr, None)
        if attr == "hinge_mask" and mem is None:                   # atom.py:597
            continue
        src = a[arg]
        if arg == "mask":
            src = src[0, ...]                                      # lwl.py:469
        if kind == FIRST:
            out.append((mem, src, 0, op))
        else:
            if src is None or mem is None:
                return None
            out += [(m, x, b, op) for b, (m, x) in enumerate(zip(mem, src)) if b < B]      # the reference zips with replace_ind
    return out


def _source_ok(mem, src, device):
    if not (_memory_ok(mem) and mem.device == device):
        return False
    elems = mem.numel() // mem.shape[0]
    if isinstance(src, (int, float)):
        return elems == 1
    if not (isinstance(src, torch.Tensor) and src.dtype == torch.float32 and src.numel() == elems and src.device in (device, torch.device("cpu"))):
        return False
    if src.is_cuda and src.is_contiguous():                       # a copy made later cannot overlap
        s0, d0 = src.data_ptr(), mem.data_ptr()
        if s0 < d0 + 4 * mem.numel() and d0 < s0 + 4 * elems:
            return False
    return True


def _tamos_assemble(self, a):
    """tamos.py:515-523: the label and box sample of all objects from the two dicts"""
    sample_x = a["sample_x"]
    tl = self.target_labels[0]
    sample_y = [torch.zeros(1, tl.shape[1], tl.shape[2], tl.shape[3], device=sample_x[0].device)]
    target_box = torch.zeros(self.target_boxes.shape[1], self.target_boxes.shape[2], device=sample_x[0].device)
    for oid, label in a["sample_ys_dict"].items():
        for s, l in zip(sample_y, label):
            s[:, oid - 1:oid] = l
    for oid, box in a["target_boxes_dict"].items():
        target_box[oid - 1:oid] = box
    return dict(a, sample_y=sample_y, target_box=target_box)


_PLAN = threading.local()           # what `covered` worked out for the call the dispatcher hands to `fast` next


def make(name):
    """(covered, fast) of the class `name` of TABLE.  `covered` binds the arguments and builds the blocks and the (memory, source) pairs once
    and leaves them for `fast`, which the dispatcher calls next with the same arguments."""
    entry = TABLE[name]
    # TaMOs assembles its label and box inside the method: new device tensors of exactly the memories' slot shapes, so only the memories
    # are checked for them; KeepTrack may replace its certainty by max(c, sqrt(c)): a new tensor of one element
    late = {"TaMOs": ("target_labels", "target_boxes"), "KeepTrack": ("target_label_certainties",)}.get(name, ())
    early = Entry(entry.module, entry.rule, entry.args, tuple(r for r in entry.rows if r[0] not in late), entry.saturate)

    def plan(self, args, kw):
        a = _bind(entry, args, kw)
        if a is None or len(getattr(self, "sample_weights", ())) == 0:
            return None
        blocks = _blocks(self, entry, a)
        if blocks is None:
            return None
        device = blocks[0].weights.device
        if any(b.weights.device != device for b in blocks):
            return None
        n0 = blocks[0].weights.numel()
        if name == "TaMOs":
            tl, tb, x = self.target_labels, self.target_boxes, a["sample_x"]
            if not (len(tl) == 1 and _memory_ok(tl[0]) and tl[0].dim() == 4 and _memory_ok(tb) and tb.dim() == 3 and tl[0].device == device
                    and tb.device == device and tl[0].shape[0] == n0 == tb.shape[0] and len(x) > 0 and isinstance(x[0], torch.Tensor)
                    and x[0].device == device):
                return None
        if name == "KeepTrack":
            c, tc = a["target_label_certainty"], self.target_label_certainties
            sqrt = self.candidate_collection is None or self.candidate_collection.object_id_of_selected_candidate == 0      # keep_track.py:630
            if not (isinstance(c, torch.Tensor) and c.numel() == 1 and c.dtype == torch.float32 and c.device in (device, torch.device("cpu"))
                    or isinstance(c, (int, float)) and not sqrt):
                return None                                            # a Python float under torch.max: the reference raises, let it
            if not (_memory_ok(tc) and tc.device == device and tc.shape[0] == n0 == tc.numel()):
                return None
        pairs = _pairs(self, early, a)
        if pairs is None or len(pairs) + len(late) > _L.PT_MEM_MAX_ROWS:
            return None
        if not all(_source_ok(m, s, device) and m.shape[0] == blocks[b].weights.numel() for m, s, b, _ in pairs):
            return None
        return a, blocks, pairs

    def covered(self, *args, **kw):
        p = plan(self, args, kw)
        _PLAN.value = None if p is None else (self, args, kw, p)
        return p is not None

    def fast(self, *args, **kw):
        stash, _PLAN.value = getattr(_PLAN, "value", None), None
        if (stash is not None and stash[0] is self and len(stash[1]) == len(args) and all(x is y for x, y in zip(stash[1], args))
                and stash[2].keys() == kw.keys() and all(stash[2][k] is kw[k] for k in kw)):
            a, blocks, pairs = stash[3]
        else:                                                          # called on its own, not through the dispatcher
            a, blocks, pairs = plan(self, args, kw)
        if name == "TaMOs":
            a = _tamos_assemble(self, a)
        if name == "KeepTrack":
            c = a["target_label_certainty"]
            if self.candidate_collection is None or self.candidate_collection.object_id_of_selected_candidate == 0:     # keep_track.py:630
                c = torch.max(c, torch.sqrt(c.clone().detach()))
            a = dict(a, target_label_certainty=c)
        if late:                                                       # the reference's order of statements
            pairs = _pairs(self, entry, a)
        device = blocks[0].weights.device
        rows, keep = [], []
        for mem, src, b, op in pairs:
            if isinstance(src, (int, float)):
                rows.append(Row(None, mem, b, SCALAR, float(src)))
                continue
            src = src.detach().to(device).contiguous()           # a CPU box or label is uploaded as the reference's assignment does
            keep.append(src)
            rows.append(Row(src, mem, b, op, float(self.params.hinge_threshold) if op == THRESH else 0.0))
        replace_ind = run(blocks, rows)
        self.previous_replace_ind = replace_ind
        if name == "KeepTrack":
            _keep_track_order(self, replace_ind)
        if entry.saturate:
            self.num_stored_samples = [n + 1 if n < self.params.sample_memory_size else n for n in self.num_stored_samples]      # lwl.py:471
        else:
            self.num_stored_samples += 1

    return covered, fast


def _keep_track_order(self, replace_ind):
    """keep_track.py:655-663, on the CPU tensor as the reference keeps it"""
    if replace_ind[0] >= len(self.mem_sort_indices):
        self.mem_sort_indices = torch.cat([self.mem_sort_indices, torch.zeros(1, dtype=torch.long)])
        self.mem_sort_indices[replace_ind[0]] = torch.max(self.mem_sort_indices) + 1
    else:
        idx = torch.nonzero(self.mem_sort_indices == replace_ind[0])
        mem_temp = self.mem_sort_indices.clone()
        mem_temp[idx:-1] = self.mem_sort_indices[idx + 1:]
        mem_temp[-1] = replace_ind[0]
        self.mem_sort_indices = mem_temp
