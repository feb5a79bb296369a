"""The project's correctness bound, once.  A device output lies within

    bound(ref_err, factor, floor) = factor * max(ref_err, floor)

of `want`, the float64 run of a restatement, where `ref_err` is the same restatement's own fp32 distance from float64 on that very case
(what fp32 arithmetic costs there in an order of summation nobody tuned) and `floor`, where a test has one, is one fp32 ulp of the
output's range.  FACTOR = 4 is defined here and nowhere else; the seeded-defect CPU tests (tests/test_fused_bounds_cpu.py and its kin) fail
if it is raised until their mutants pass.  A module whose measured device error on the MI355X exceeds FACTOR / 2 states its worst measured
ratio and takes raised_factor() of it.

Two floors exist and are deliberately NOT unified:

    ulp_of_max(want)     = 2^-23 * max|want|                      (eco, eco_init, seg_readout)
    spacing_of_max(want) = np.spacing(np.float32(max|want|))      (fast passes, box encoders)

spacing_of_max is never larger than ulp_of_max and up to 2 x smaller (it is 2^-23 times the power of two at or below max|want|).  Every
test keeps the floor it was written and measured with: moving one to the smaller floor tightens its bound with no device evidence
(box_enc sits at 3.02 of 4), moving one to the larger floor weakens it.  A later change that has the device tables in hand may unify them.

anchor() runs a restatement once in float64 and once in fp32 and caches the pair; held() is the single print, record and assert; Table
writes the recorded rows to the file an environment variable names.  numpy only at import: torch is touched only when a tensor is passed
in.  Reads nothing outside the repository.  Test infrastructure only."""
import math
import os
from collections import OrderedDict, namedtuple

import numpy as np

FACTOR = 4
ULP = 2.0 ** -23                                   # one fp32 ulp of 1
# The CPU convolutions block their sums by the number of threads, so the fp32 run's rounding -- ref_err -- moves by tens of per cent with
# it.  The goldens' ref_fp32_err were written with 8 threads; a torch anchor pins its fp32 run to that (anchor(threads=THREADS)) so that
# ref_err does not follow the ambient thread count (a CPU with another vector width may still round differently:
# tests/test_fused_bounds_cpu.py compares with the goldens).
THREADS = 8
# want: {output: float64 numpy, read-only}; f32: the fp32 run as `run` returned it; ref_err: float, or {group: float} when grouped;
# ref_errs: {output: float}
Anchor = namedtuple("Anchor", "want f32 ref_err ref_errs")
_CACHE = {}


def raised_factor(worst_measured, f_max):
    """FACTOR where the worst measured device ratio stays at or below half of it; otherwise twice that ratio, rounded up (the 2 covers the
    tens of per cent by which ref_err itself moves with the summation blocking), and never above f_max, below which the module's weakest
    seeded defect still has to fail."""
    f = FACTOR if worst_measured <= FACTOR / 2 else math.ceil(2 * worst_measured)
    assert FACTOR <= f <= f_max, (worst_measured, f, f_max)
    return f


def host(t):
    """float64 numpy of a tensor (any device) or of anything numpy reads"""
    return t.detach().double().cpu().numpy() if hasattr(t, "detach") else np.asarray(t, dtype=np.float64)


def dev(a, device="cuda:0", dtype=None):
    """the array on the device (None stays None)"""
    import torch
    if a is None:
        return None
    a = np.asarray(a)
    if not (a.flags.c_contiguous and a.flags.writeable):           # torch wants both of the host array; a read-only `want` or input is copied
        a = np.array(a, order="C")
    return torch.from_numpy(a).to(device=device, dtype=dtype)


def __getattr__(name):
    if name == "needs_bundle":                     # resolved on use: pytest and the harness are not needed by the tools
        import pytest
        from oracle import ref_harness
        return pytest.mark.skipif(not ref_harness.available(), reason="no reference tree / bundle (oracle/_ref)")
    raise AttributeError(name)


def _max_abs(want):
    return max(float(np.abs(host(w)).max()) for w in (want.values() if isinstance(want, dict) else (want,)))


def ulp_of_max(want):
    return ULP * _max_abs(want)


def spacing_of_max(want):
    return float(np.spacing(np.float32(_max_abs(want))))


def bound(ref_err, factor=FACTOR, floor=0.0):
    return factor * max(float(ref_err), floor)


def errors(want, got):
    """{output: max |got - want|} for arrays or tensors `got` against an Anchor's `want`; one array against one array: {"": error}."""
    if not isinstance(want, dict):
        want, got = {"": host(want)}, {"": got}
    return OrderedDict((q, float(np.abs(host(got[q]).reshape(w.shape) - w).max())) for q, w in want.items())


def by_group(errs, group):
    """{group: largest error of its outputs}"""
    out = OrderedDict()
    for q, e in errs.items():
        out[group(q)] = max(out.get(group(q), 0.0), e)
    return out


def anchor(key, run, group=None, threads=None):
    """Anchor of `run(dtype) -> OrderedDict {output: array or tensor}`, called once with np.float64 and once with np.float32, computed once
    per session under `key`.  group: output -> group name; ref_err is then per group.  threads: the torch thread count of the fp32 run (see
    THREADS)."""
    if key not in _CACHE:
        f64 = run(np.float64)
        assert all(str(v.dtype).endswith("float64") for v in f64.values()), {q: v.dtype for q, v in f64.items()}
        if threads is None:
            f32 = run(np.float32)
        else:
            import torch
            ambient = torch.get_num_threads()
            try:
                torch.set_num_threads(threads)
                f32 = run(np.float32)
            finally:
                torch.set_num_threads(ambient)
        assert all(str(v.dtype).endswith("float32") for v in f32.values()), {q: v.dtype for q, v in f32.items()}     # the fp32 run stays fp32
        want = OrderedDict((q, host(v)) for q, v in f64.items())
        for w in want.values():
            w.setflags(write=False)
        errs = errors(want, f32)
        _CACHE[key] = Anchor(want, f32, max(errs.values()) if group is None else by_group(errs, group), errs)
    return _CACHE[key]


def _rows(errs, ref_err, floor, group):
    """per output (output, err, its ref_err, unit = max(ref_err, floor), err / unit); a zero unit with zero error is ratio 0"""
    for q, e in errs.items():
        r = float(ref_err[group(q) if group else q] if isinstance(ref_err, dict) else ref_err)
        unit = max(r, floor)
        yield q, e, r, unit, (e / unit if unit > 0 else 0.0 if e == 0 else math.inf)


def within(errs, ref_err, factor=FACTOR, floor=0.0, group=None):
    """every output within the bound of its (group's) ref_err"""
    return all(e <= factor * unit for _, e, _, unit, _ in _rows(errs, ref_err, floor, group))


def report(tag, errs, ref_err, factor=FACTOR, floor=0.0, group=None):
    """The line every test prints before it asserts: per output the measured error and its ratio to max(ref_err, floor)."""
    refs = " ".join(f"{g} {r:.3e}" for g, r in ref_err.items()) if isinstance(ref_err, dict) else f"{float(ref_err):.3e}"
    return (f"\n{tag}: max |out - float64| " + "  ".join(f"{q} {e:.3e} ({x:.2f}x)".lstrip() for q, e, _, _, x in _rows(errs, ref_err, floor, group))
            + f"  ref_err {refs}, floor {floor:.3e}; bound {factor} x max(ref_err, floor)")


def held(tag, errs_or_got, want, ref_err, factor=FACTOR, floor=0.0, flat=None, table=None, star=False, group=None, msg=""):
    """Print, record and assert the float64 bound.  errs_or_got: {output: error}, or the outputs themselves ({output: array or tensor}, or
    one array or tensor with `want` one array) to measure against `want`.  ref_err: float, or {group: float} looked up through `group`.
    floor: a number, or ulp_of_max / spacing_of_max to take of `want`.  flat: an absolute bound held as well.  table: a Table that takes
    one row per output (star: the row's tag is marked *).  msg: appended to the assertion message.  -> {output: error}"""
    if callable(floor):
        floor = floor(want)
    if isinstance(errs_or_got, dict) and all(isinstance(v, float) for v in errs_or_got.values()):
        errs = errs_or_got
    else:
        errs = errors(want, errs_or_got)
    print(report(tag, errs, ref_err, factor, floor, group) + (f" and {flat:.3e}" if flat is not None else ""))
    rows = list(_rows(errs, ref_err, floor, group))
    if table is not None:
        for q, e, r, _, x in rows:
            table.row(f"{tag} {q}".rstrip() + ("*" if star else ""), e, r, floor, x)
    for q, e, r, unit, x in rows:
        assert e <= factor * unit, f"{tag} {q}: {e:.3e} = {x:.2f} x max(ref_err {r:.3e}, floor {floor:.3e}), bound {factor} x = {factor * unit:.3e}\n{msg}"
        assert flat is None or e <= flat, f"{tag} {q}: {e:.3e} above the flat bound {flat:.3e}\n{msg}"
    return errs


class Table:
    """The rows `tag err ref_err floor ratio` of one module, written under `header` to the file the environment variable names -- on every
    row, so that a run that stops early leaves what it measured -- and nowhere when the variable is not set."""

    def __init__(self, env_var, header):
        self.env_var, self.header, self.rows = env_var, header, OrderedDict()

    def row(self, tag, err, ref_err, floor, ratio, bounded=True):
        """bounded=False: a row whose ratio is not held to a factor and does not enter the worst ratio"""
        self.rows[tag] = (float(err), float(ref_err), float(floor), float(ratio), bounded)
        path = os.environ.get(self.env_var)
        if not path:
            return
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        width = max(44, max(len(k) for k in self.rows))
        with open(path, "w") as fh:
            fh.write(self.header.rstrip("\n") + f"\n{'case':{width}s} {'err':>10s} {'ref_err':>10s} {'floor':>10s} {'ratio':>7s}\n")
            for k, (e, r, f, x, _) in self.rows.items():
                fh.write(f"{k:{width}s} {e:10.3e} {r:10.3e} {f:10.3e} {x:7.2f}\n")
            worst = [x for _, _, _, x, b in self.rows.values() if b]
            if worst:
                fh.write(f"worst ratio: {max(worst):.2f}\n")
