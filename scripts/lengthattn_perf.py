#!/usr/bin/env python
"""Timing of the length-attention kernel (csrc/jg_lengthattn.hip), for DESIGN.md 3.7 and profiles/lengthattn_perf.json.

The op has no profiling class of its own (JG_PROF_CLASSES is pinned), so its launch is timed from outside, by HIP events
on a stream handed to ``jg_forward``: the conv stack of axial500 with ONE stand-alone ``transformer_encoder`` behind it
beside the same stack with FIVE, device-resident ids and outputs, interleaved passes at the default launch group - the
difference of the two event times over the four extra launches per launch group is one launch.  Per arithmetic of the
surrounding program:

* microseconds per length-attention launch;
* TFLOP/s of all its matrix products (``jg_model_flops_per_window``: the dense products, k and v once per query tile, plus
  4 L^2 C of scores and context) against the 157.3 TFLOP/s exact-f32 matrix-core peak - the scores and the context run on
  the vector ALUs in this first form of the kernel, the figure says what the launch achieves, not which unit did it;
* the multiple of the HBM floor 2 x 4 B x 6 L C per window over the device-to-device copy rate measured first;
* end-to-end Mbp/s (encode + forward) of axial500 beside crossframe500 and baseline500, in interleaved runs.

Usage: python scripts/lengthattn_perf.py [--windows 12288] [--group 6144] [--repeats 5] [--out profiles/lengthattn_perf.json]
"""
import argparse
import copy
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "scripts"))

from frameattn_perf import F32_MFMA_PEAK_TFLOPS, copy_rate_gbs  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=12288)
    ap.add_argument("--group", type=int, default=6144, help="windows per launch group (6144: the default at 166 positions)")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import yaml

    from jaeger_amd import _lib as L
    from jaeger_amd.engine import JaegerHipEngine
    from jaeger_amd.plan import build_plan
    from jaeger_amd.weights import random_weights
    fsize, n_win = 500, args.windows
    groups = -(-n_win // args.group)
    res = {"windows": n_win, "fsize": fsize, "windows_per_launch_group": args.group, "copy_rate_gbs": round(copy_rate_gbs(), 1)}
    golden = lambda name: yaml.safe_load((ROOT / "tests" / "golden" / f"{name}_project.yaml").read_text())["model"]

    def encoders(n):
        """axial500's conv stack with n stand-alone encoders of the axial layer's sizes in the layer's place."""
        cfg = copy.deepcopy(golden("axial500"))
        layers = cfg["representation_learner"]["hidden_layers"]
        at = [i for i, l in enumerate(layers) if l["name"] == "axial_attention"][0]
        a = layers[at]["config"]
        enc = {"name": "transformer_encoder", "config": {k: a[k] for k in ("embed_dim", "num_heads", "feed_forward_dim")}}
        layers[at:at + 1] = [copy.deepcopy(enc) for _ in range(n)]
        return cfg

    def engine(cfg, precision):
        return JaegerHipEngine(model_cfg=cfg, weights=random_weights(build_plan(cfg)), device_id=0, precision=precision)

    stream = torch.cuda.Stream()
    gen = torch.Generator(device="cuda").manual_seed(20261018)

    def event_ms(eng, ids, out):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        L.check(eng.model.lib.jg_forward(eng.model.handle, ids.data_ptr(), L.JG_PTR_DEVICE, ids.shape[0], ids.shape[2],
                                         out.data_ptr(), None, None, None, L.JG_PTR_DEVICE, args.group, stream.cuda_stream), "jg_forward")
        e1.record(stream)
        stream.synchronize()
        return e0.elapsed_time(e1)

    few, many = 1, 5
    for precision in ("f32", "f16x3"):
        legs = {n: engine(encoders(n), precision) for n in (few, many)}
        l = legs[few].model.row_length(fsize)
        c = [x for x in legs[few].plan.rep if type(x).__name__ == "LengthAttn"][0].channels
        ids = torch.randint(1, 65, (n_win, 6, l), dtype=torch.uint8, device="cuda", generator=gen)
        out = torch.empty((n_win, legs[few].model.widths["prediction"]), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        for eng in legs.values():                      # warm-up: workspace, code objects
            event_ms(eng, ids, out)
        ms = {n: [] for n in legs}
        for _ in range(args.repeats):                  # interleaved
            for n, eng in legs.items():
                ms[n].append(event_ms(eng, ids, out))
        launches = (many - few) * groups
        us = (float(np.median(ms[many])) - float(np.median(ms[few]))) * 1e3 / launches
        flops = (legs[many].model.flops_per_window(l) - legs[few].model.flops_per_window(l)) / (many - few) * args.group
        floor_us = 2 * 4 * 6 * l * c * args.group / (res["copy_rate_gbs"] * 1e9) * 1e6
        res[precision] = {"us_per_launch": round(us, 1), "positions_per_frame": l, "channels": c,
                          "pass_ms": {f"{n} encoders": [round(v, 3) for v in ms[n]] for n in ms},
                          "matrix_product_gflop_per_launch": round(flops / 1e9, 2),
                          "tflops": round(flops / (us * 1e-6) / 1e12, 2),
                          "fraction_of_f32_mfma_peak": round(flops / (us * 1e-6) / 1e12 / F32_MFMA_PEAK_TFLOPS, 4),
                          "hbm_floor_us": round(floor_us, 1), "multiple_of_hbm_floor": round(us / floor_us, 1)}
        for eng in legs.values():
            eng.close()
        del ids, out

    # end to end, interleaved
    rng = np.random.Generator(np.random.PCG64(20261017))
    seq = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, fsize * n_win)].copy()
    starts = (np.arange(n_win) * fsize).astype(np.int64)
    lens = np.full(n_win, fsize, np.int32)
    legs = {f"{name} {precision}": engine(golden(name), precision)
            for name in ("axial500", "crossframe500", "baseline500") for precision in ("f16x3", "f32")}
    want = ("prediction",)
    for eng in legs.values():
        eng.predict_windows(seq, starts, lens, fsize, want=want)
    times = {k: [] for k in legs}
    for _ in range(args.repeats):
        for k, eng in legs.items():
            t0 = time.perf_counter()
            eng.predict_windows(seq, starts, lens, fsize, want=want)
            times[k].append(time.perf_counter() - t0)
    res["end_to_end_mbps"] = {k: {"median": round(n_win * fsize / float(np.median(v)) / 1e6, 1),
                                  "runs": [round(n_win * fsize / t / 1e6, 1) for t in v]} for k, v in times.items()}
    for eng in legs.values():
        eng.close()
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
