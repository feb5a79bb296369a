"""ECO's Fourier-domain per-frame path on one MI355X, per operation, at the default parameter set (pytracking/parameter/eco/default.py:
S = 5 scales; shallow block 96 -> 16 channels on 60 x 60, deep block 256 -> 64 on 15 x 15; 240 x 240 score grid; n = 200 samples):
    python -B tools/bench_eco.py [--rounds N] [--out profiles/eco_bench.json]
  sample_shallow / sample_deep   pytracking_amd.eco.sample_transform (one launch)                    vs  projection, window, torch.fft, factors
  apply                          pytracking_amd.eco.apply_filter, both blocks                        vs  complex products + channel sum
  localize                       pytracking_amd.eco.localize, both blocks, 'weightedsum' (4 launches) vs  sum, zero padding, torch.fft.irfftn, max2d
  insert                         pytracking_amd.eco.insert with a shift, both blocks                 vs  shift_fs + the slot assignment
  frame                          all of the above in ECO.track's order, without the host read of the arg-max
  filter_update                  pytracking_amd.eco.filter_update, both blocks, 5 CG iterations, Polak-Ribiere, the direction carried over
                                 (23 launches)  vs  the reference's own FilterOptim.run (tracker/eco/optim.py) on the same tensors, when the
                                 reference tree or its bundle is there (`filter_update_stock` says); also `sample_memory_bytes` = 8 Hf Wh n c
                                 summed over the blocks and `over_one_pass_at_8TBps` = device time / (those bytes / 8 TB/s)
`stock` is the reference's sequence of operations in stock PyTorch-ROCm on `torch.fft` on the same GPU (pytracking_amd.eco's torch forms:
the reference's own fourier.py cannot run on the installed torch).  Both variants of a
case are interleaved in ONE process: every round times each once, so clock and thermal drift hit them alike.  Two figures per variant:
`device_us` = event-timed batch of 20 back-to-back calls / 20 (what the GPU spends), `host_us` = one call + synchronisation, host clock.
Medians over the rounds."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pytracking_amd import eco, synth  # noqa: E402

DEV = "cuda:0"
BATCH = 20
S, N, GRID, WEIGHTS, SHIFT = 5, 200, (240, 240), (0.4, 0.6), (0.11, -0.07)
BLOCKS = {"shallow": (96, 16, 60, 60), "deep": (256, 64, 15, 15)}          # Cin, c, H, W


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eco_bench.json"))
    a = ap.parse_args()
    dv = lambda t: torch.from_numpy(t).to(DEV)      # noqa: E731
    res = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "batch": BATCH, "scales": S, "samples": N, "grid": list(GRID),
           "blocks": {k: list(v) for k, v in BLOCKS.items()}, "stock_kind": "pytracking_amd.eco torch forms on torch.fft",
           "cases": {}}
    blk = {}
    for b, (name, (Cin, c, H, W)) in enumerate(BLOCKS.items()):
        interp = synth.eco_interp(9100 + b, H, W)
        Hf, Wh = eco.series_sizes(H, W)
        blk[name] = dict(x=dv(synth.eco_features(9000 + b, S, Cin, H, W)), P=dv(synth.eco_projection(9010 + b, Cin, c)), win=dv(synth.eco_window(H, W)),
                         interp=(dv(interp[0]), dv(interp[1])), hf=dv(synth.eco_series(9020 + b, 1, c, Hf, Wh)),
                         mem=torch.zeros(Hf, Wh, N, c, 2, device=DEV))
    names = list(BLOCKS)

    def transform(form, k):
        d = blk[k]
        return form(d["x"], d["P"], d["win"], d["interp"])

    with torch.no_grad():
        xf = {k: transform(eco.sample_transform, k) for k in names}
        sf = {k: eco.apply_filter(blk[k]["hf"], xf[k]) for k in names}

        def frame(tr, ap_, loc, ins):
            x = [transform(tr, k) for k in names]
            out = loc([ap_(blk[k]["hf"], e) for k, e in zip(names, x)], WEIGHTS, GRID)
            for k, e in zip(names, x):
                ins(blk[k]["mem"], e[2:3], 7, SHIFT)
            return out[0]

        cases = {
            "sample_shallow": (lambda: transform(eco.sample_transform, "shallow"), lambda: transform(eco.sample_transform_torch, "shallow")),
            "sample_deep": (lambda: transform(eco.sample_transform, "deep"), lambda: transform(eco.sample_transform_torch, "deep")),
            "apply": (lambda: [eco.apply_filter(blk[k]["hf"], xf[k]) for k in names][0],
                      lambda: [eco.apply_filter_torch(blk[k]["hf"], xf[k]) for k in names][0]),
            "localize": (lambda: eco.localize([sf[k] for k in names], WEIGHTS, GRID)[0],
                         lambda: eco.localize_torch([sf[k] for k in names], WEIGHTS, GRID)[0]),
            "insert": (lambda: [eco.insert(blk[k]["mem"], xf[k][2:3], 7, SHIFT) for k in names][0][:, :, 7],
                       lambda: [eco.insert_torch(blk[k]["mem"], xf[k][2:3], 7, SHIFT) for k in names][0][:, :, 7]),
            "frame": (lambda: frame(eco.sample_transform, eco.apply_filter, eco.localize, eco.insert),
                      lambda: frame(eco.sample_transform_torch, eco.apply_filter_torch, eco.localize_torch, eco.insert_torch)),
        }
        # filter update: deployed blocks, memories with a spectrum's decay, steady-state weights
        import numpy as np
        fu = dict(filters=[], samples=[], weights=[], yf=[], regs=[], energy=[], new_xf=[], lrs=[0.025, 0.0075], reg_energy=[])
        for b, (k, (Rh, Rw)) in enumerate(zip(names, ((5, 5), (3, 3)))):
            Cin, c, H, W = BLOCKS[k]
            Hf, Wh = eco.series_sizes(H, W)
            mem = synth.eco_series(9200 + b, N, c, Hf, Wh)
            fu["samples"].append(dv(np.ascontiguousarray(mem.transpose(2, 3, 0, 1, 4))))
            fu["weights"].append(dv(synth.decay_weights(N, fu["lrs"][b])))
            ky, kx = np.arange(Hf) - (Hf - 1) // 2, np.arange(Wh)
            fu["yf"].append(dv((np.exp(-0.5 * (ky[:, None] / 2.0) ** 2 - 0.5 * (kx[None, :] / 2.0) ** 2) / (Hf * W)).astype(np.float32).reshape(1, 1, Hf, Wh)))
            reg = np.full((Rh, Rw), 0.004, dtype=np.float32)
            reg[Rh // 2, Rw // 2] = 0.05
            fu["regs"].append(dv(reg.reshape(1, 1, Rh, Rw)))
            fu["reg_energy"].append(float((reg.astype(np.float64) ** 2).sum()))
            fu["energy"].append(dv(np.ascontiguousarray((mem ** 2).sum(-1).mean(0, keepdims=True))))
            fu["filters"].append(dv(synth.eco_series(9210 + b, 1, c, Hf, Wh) * np.float32(0.01)))
            fu["new_xf"].append(dv(synth.eco_series(9220 + b, 1, c, Hf, Wh)))
        forget = (1 - 0.025) ** 75
        state = eco.new_cg_state(fu["filters"])
        mem_bytes = sum(8 * s.shape[0] * s.shape[1] * s.shape[2] * s.shape[3] for s in fu["samples"])

        def fused_update():
            eco.filter_update(fu["filters"], fu["samples"], fu["weights"], fu["yf"], fu["regs"], fu["energy"], fu["new_xf"], state, 5, fu["lrs"],
                              fu["reg_energy"], False, True, forget)
            return fu["filters"][0]
        stock_update, res["filter_update_stock"] = fused_update, "absent (no reference tree or bundle): the stock column repeats the kernels"
        try:
            from oracle import ref_harness
            if ref_harness.available():
                ref_harness.install()
                import types
                from pytracking import TensorList
                from pytracking.tracker.eco.optim import FilterOptim
                prm = types.SimpleNamespace(fletcher_reeves=False, standard_alpha=True, direction_forget_factor=forget, debug=0,
                                            precond_learning_rate=TensorList(fu["lrs"]), precond_data_param=0.3, precond_reg_param=0.15)
                opt = FilterOptim(prm, TensorList([torch.tensor(v, device=DEV) for v in fu["reg_energy"]]))
                opt.register(TensorList([f.clone() for f in fu["filters"]]), TensorList(fu["samples"]), TensorList(fu["yf"]),
                             TensorList(fu["weights"]), TensorList(fu["regs"]))
                opt.sample_energy = TensorList([e.clone() for e in fu["energy"]])

                def stock_update():
                    opt.run(5, TensorList(fu["new_xf"]))
                    return opt.filter[0]
                res["filter_update_stock"] = "the reference's FilterOptim.run in stock PyTorch on the same GPU"
        except Exception as exc:      # noqa: BLE001
            res["filter_update_stock"] = f"absent ({type(exc).__name__}): the stock column repeats the kernels"
        cases["filter_update"] = (fused_update, stock_update)
        for name, (fused, stock) in cases.items():
            variants = {"fused": fused, "stock": stock}
            diff = float((fused() - stock()).abs().max())
            for fn in variants.values():
                for _ in range(5):
                    fn()
            torch.cuda.synchronize()
            dev_t, host_t = {k: [] for k in variants}, {k: [] for k in variants}
            for _ in range(a.rounds):
                for k, fn in variants.items():
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(BATCH):
                        fn()
                    e1.record()
                    torch.cuda.synchronize()
                    dev_t[k].append(e0.elapsed_time(e1) * 1e3 / BATCH)
                    t0 = time.perf_counter()
                    fn()
                    torch.cuda.synchronize()
                    host_t[k].append((time.perf_counter() - t0) * 1e6)
            out = {"max_abs_fused_minus_stock": diff}
            for k in variants:
                out[k] = {"device_us": statistics.median(dev_t[k]), "device_us_min": min(dev_t[k]), "host_us": statistics.median(host_t[k])}
            out["stock_over_fused_device"] = out["stock"]["device_us"] / out["fused"]["device_us"]
            out["stock_over_fused_host"] = out["stock"]["host_us"] / out["fused"]["host_us"]
            if name == "filter_update":
                out["sample_memory_bytes"] = mem_bytes
                out["over_one_pass_at_8TBps"] = out["fused"]["device_us"] / (mem_bytes / 8e12 * 1e6)
            res["cases"][name] = out
            print(name, json.dumps(out), flush=True)
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
