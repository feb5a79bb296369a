"""ATOM's per-frame score localisation on one MI355X at the deployed size (18 x 18 raw scores -> 288 x 288 grid, 4 x 4 kernel, advanced
localisation, no output window), for S = 1 and S = 5 scales:
    python -B tools/bench_atom_localize.py [--rounds N] [--out profiles/atom_localize_bench.json]
  fused   pytracking_amd.atom_localize.localize: two launches (k_loc_interp, k_loc_decide) and one polled wait
  stock   the reference's sequence (pytracking/tracker/atom/atom.py:304-406 with fourier.cfft2 / shift_fs / sample_fs) restated on torch.fft
          with stock PyTorch-ROCm operators on the SAME GPU: rfftn, the shift by concatenation, the phase factors, zero padding, irfftn,
          four torch.cat rolls, two max2d's, a clone, a masked fill and the .item() / .cpu() round trips
`stock` is this project's own restatement: it reads no reference file (the reference itself cannot run on the installed torch: torch.rfft
is gone).  Both variants are interleaved in ONE process: every round times each once, so clock and thermal drift hit them alike.  Two figures
per variant: `host_us` = one call until its results are on the host, host clock; `device_us` = event-timed batch of 20 back-to-back calls
/ 20 (for `stock` that includes the gaps its synchronisations leave).  Medians over the rounds, with the minimum and the quartiles."""
import argparse
import json
import math
import os
import statistics
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pytracking_amd import atom_localize as AL  # noqa: E402

DEV = "cuda:0"
BATCH = 20
N, G, KERNEL = 18, 288, (4, 4)
PRM = dict(target_not_found_threshold=0.25, distractor_threshold=0.8, hard_negative_threshold=0.5, target_neighborhood_scale=2.2, dispalcement_scale=0.8)
TARGET_SZ, TARGET_SCALE = (40.0, 33.0), 1.25


def scores(S, seed=3):
    rng = np.random.default_rng(seed)
    s = 0.05 + 0.01 * rng.standard_normal((S, 1, N, N))
    r, c = np.mgrid[0:N, 0:N]
    for k in range(S):
        for (r0, c0, a) in ((10, 8, 1.0 - 0.03 * abs(k - S // 2)), (4, 13, 0.55)):
            s[k, 0] += a * np.exp(-((r - r0) ** 2 + (c - c0) ** 2) / (2 * 1.2 ** 2))
    return torch.from_numpy(s.astype(np.float32)).to(DEV)


def max2d(a):
    mv, ar = torch.max(a, dim=-2)
    mv, ac = torch.max(mv, dim=-1)
    ar = ar.gather(-1, ac.unsqueeze(-1)).squeeze(-1)
    return mv, torch.stack((ar, ac), -1)


def stock_localize(s):
    """atom.py:306-313 and :341-406 on a (S, 1, N, N) device tensor, complex tensors in place of the trailing dimension of 2"""
    out_sz = torch.Tensor([G, G])
    support = torch.Tensor([G, G])
    sf = torch.fft.rfftn(1.0 * s, dim=(-2, -1))
    h = sf.shape[2] + 2
    sf = torch.cat((sf[:, :, (h - 1) // 2:], sf[:, :, :h // 2]), 2) / (s.size(2) * s.size(3))                      # rfftshift2
    shift = math.pi * (1 - torch.Tensor([KERNEL[0] % 2, KERNEL[1] % 2]) / torch.Tensor([N, N]))
    ky = torch.arange(-int((sf.shape[2] - 1) / 2), int(sf.shape[2] / 2 + 1), dtype=torch.float32, device=s.device).view(1, 1, -1, 1)
    kx = torch.arange(0, sf.shape[3], dtype=torch.float32, device=s.device).view(1, 1, 1, -1)
    sf = sf * torch.polar(torch.ones_like(ky), shift[0].item() * ky) * torch.polar(torch.ones_like(kx), shift[1].item() * kx)
    sz = (sf.shape[2], 2 * sf.shape[3] - 1)
    tot = (G - sz[0], G - sz[1])
    top = int(tot[0] / 2)
    sf = F.pad(sf, (0, int((tot[1] + 1) / 2), top, tot[0] - top))
    mid = int((sf.shape[2] - 1) / 2)
    sc = G * G * torch.fft.irfftn(torch.cat((sf[:, :, mid:], sf[:, :, :mid]), 2), s=(G, G), dim=(-2, -1))         # sample_fs
    sc = torch.cat([sc[..., (G + 1) // 2:, :], sc[..., :(G + 1) // 2, :]], -2)
    sc = torch.cat([sc[..., :, (G + 1) // 2:], sc[..., :, :(G + 1) // 2]], -1)
    m1, d1 = max2d(sc)
    _, scale_ind = torch.max(m1, dim=0)
    m1 = m1[scale_ind]
    d1 = d1[scale_ind, ...].float().cpu().view(-1)
    t1 = d1 - out_sz // 2
    tv1 = t1 * (support / out_sz) * TARGET_SCALE
    if m1.item() < PRM["target_not_found_threshold"]:
        return tv1, scale_ind, sc, "not_found"
    neigh = PRM["target_neighborhood_scale"] * torch.Tensor(TARGET_SZ) / TARGET_SCALE
    t = max(round(d1[0].item() - neigh[0].item() / 2), 0)
    b = min(round(d1[0].item() + neigh[0].item() / 2 + 1), G)
    le = max(round(d1[1].item() - neigh[1].item() / 2), 0)
    r = min(round(d1[1].item() + neigh[1].item() / 2 + 1), G)
    masked = sc[scale_ind:scale_ind + 1, ...].clone()
    masked[..., t:b, le:r] = 0
    m2, d2 = max2d(masked)
    d2 = d2.float().cpu().view(-1)
    t2 = d2 - out_sz // 2
    tv2 = t2 * (support / out_sz) * TARGET_SCALE
    if m2 > PRM["distractor_threshold"] * m1:
        n1, n2 = torch.sqrt(torch.sum(t1 ** 2)), torch.sqrt(torch.sum(t2 ** 2))
        th = PRM["dispalcement_scale"] * math.sqrt(G * G) / 2
        if n2 > th and n1 < th:
            return tv1, scale_ind, sc, "hard_negative"
        if n2 < th and n1 > th:
            return tv2, scale_ind, sc, "hard_negative"
        return tv1, scale_ind, sc, "uncertain"
    if m2 > PRM["hard_negative_threshold"] * m1 and m2 > PRM["target_not_found_threshold"]:
        return tv1, scale_ind, sc, "hard_negative"
    return tv1, scale_ind, sc, None


def quartiles(v):
    q = statistics.quantiles(v, n=4)
    return {"median": statistics.median(v), "min": min(v), "q1": q[0], "q3": q[2]}


def time_variants(variants, rounds):
    """variants {name: fn}; every fn returns with its results on the host"""
    for fn in variants.values():
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    dev_t, host_t = {k: [] for k in variants}, {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(BATCH):
                fn()
            e1.record()
            torch.cuda.synchronize()
            dev_t[k].append(e0.elapsed_time(e1) * 1e3 / BATCH)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            host_t[k].append((time.perf_counter() - t0) * 1e6)
    return {k: {"host_us": quartiles(host_t[k]), "device_us": quartiles(dev_t[k])} for k in variants}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "atom_localize_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_atom_localize needs the GPU")
    res = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "batch": BATCH, "series": [N, N], "grid": [G, G],
           "stock_kind": "this project's restatement of the reference's sequence on torch.fft, stock torch operators on the same GPU", "cases": {}}
    with torch.no_grad():
        for S in (1, 5):
            s = scores(S)
            st = AL.state_block(kernel_size=KERNEL, output_sz=(G, G), img_support_sz=(G, G), target_sz=TARGET_SZ, target_scale=TARGET_SCALE,
                                scale_factors=[1.02 ** (k - S // 2) for k in range(S)], advanced_localization=True, **PRM)
            fused = lambda: AL.localize(s, st)  # noqa: E731
            stock = lambda: stock_localize(s)  # noqa: E731
            f, k = fused(), stock()
            agree = f.flag == k[3] and int(f.scale_ind) == int(k[1]) and f.translation_vec.tolist() == k[0].tolist()
            diff = float((f.scores - k[2]).abs().max())
            out = time_variants({"fused": fused, "stock": stock}, a.rounds)
            out.update(scales=S, flag=str(f.flag), outcome_agrees=bool(agree), max_abs_map_fused_minus_stock=diff)
            out["stock_over_fused_host"] = out["stock"]["host_us"]["median"] / out["fused"]["host_us"]["median"]
            out["stock_over_fused_device"] = out["stock"]["device_us"]["median"] / out["fused"]["device_us"]["median"]
            res["cases"][f"s{S}"] = out
            print(f"s{S}", json.dumps(out), flush=True)
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
