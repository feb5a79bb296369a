"""torch.rfft / torch.irfft as pytracking/libs/fourier.py:24,31 and dcf.py:134,139 call them (removed in torch 1.8), on torch.fft: the
one-sided, unnormalised real transform over the last `signal_ndim` dimensions with complex numbers as a trailing dimension of 2, and its
normalised inverse with `signal_sizes`.  tools/make_golden_eco.py installs the two functions into `torch` before it imports the unmodified
reference, so the ECO goldens are pinned to the reference plus this shim; tests/test_eco_cpu.py checks the shim against a float64 dense
DFT.  Test infrastructure only."""
import torch


def rfft(a, signal_ndim, normalized=False, onesided=True):
    assert onesided and not normalized
    return torch.view_as_real(torch.fft.rfftn(a, dim=tuple(range(-signal_ndim, 0))))


def irfft(a, signal_ndim, normalized=False, onesided=True, signal_sizes=None):
    assert onesided and not normalized
    return torch.fft.irfftn(torch.view_as_complex(a.contiguous()), s=signal_sizes, dim=tuple(range(-signal_ndim, 0)))


def install():
    torch.rfft, torch.irfft = rfft, irfft
