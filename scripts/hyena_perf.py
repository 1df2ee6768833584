#!/usr/bin/env python
"""Timing of the hyena op (csrc/jg_hyena.hip), for DESIGN.md 3.8 and profiles/hyena_perf.json.

The op has no profiling class of its own (JG_PROF_CLASSES is pinned), so it is timed from outside, by HIP events on a
stream handed to ``jg_forward``: hyenafirst500 (embedding -> ``hyena_block`` -> max pool -> dense, the reference's own
hyena_test.yaml) with ONE block beside the same model with FIVE, device-resident ids and outputs, interleaved passes,
one launch group - the difference of the two event times over the four extra ops is one op (its 2 + order launches
together).  Per row length (166 positions: 500-bp windows; 665: 2 000-bp windows), in exact f32 (the only conv of the
model is the one-tap identity conv in front of the first block):

* microseconds per hyena op and launch group;
* the achieved rate of the op's multiply-adds (``jg_model_flops_per_window``: the projections and 2 x order x C x
  L (L + 1) / 2 of the convolutions) beside the f32 vector peak - 157.3 TFLOP/s, 64 FLOP a clock and SIMD with packed
  fmas, which is also the rate of the exact-f32 matrix cores; plain v_fma_f32, as the convolution loop issues them, reach
  half of it; the projections are a small share of the work;
* the multiple of the HBM floor: the op's unavoidable traffic, one read and one write of the (6, L, C) f32 rows per window,
  over the device-to-device copy rate measured first (the scratch traffic of this first form comes on top of the floor:
  that is what the multiple shows).

Usage: python scripts/hyena_perf.py [--windows 6144] [--repeats 5] [--out profiles/hyena_perf.json]
"""
import argparse
import copy
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "scripts"))

from frameattn_perf import copy_rate_gbs  # noqa: E402

F32_VECTOR_PEAK_TFLOPS = 157.3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=6144)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import yaml

    from jaeger_amd import _lib as L
    from jaeger_amd.engine import JaegerHipEngine
    from jaeger_amd.plan import build_plan
    from jaeger_amd.weights import random_weights
    res = {"copy_rate_gbs": round(copy_rate_gbs(), 1), "f32_vector_peak_tflops": round(F32_VECTOR_PEAK_TFLOPS, 1)}
    golden = lambda name: yaml.safe_load((ROOT / "tests" / "golden" / f"{name}_project.yaml").read_text())["model"]

    def blocks(n):
        """hyenafirst500 with n hyena blocks of the fixture's sizes in the layer's place."""
        cfg = copy.deepcopy(golden("hyenafirst500"))
        layers = cfg["representation_learner"]["hidden_layers"]
        at = [i for i, l in enumerate(layers) if l["name"] == "hyena_block"][0]
        layers[at:at + 1] = [copy.deepcopy(layers[at]) for _ in range(n)]
        return cfg

    def engine(cfg, precision):
        return JaegerHipEngine(model_cfg=cfg, weights=random_weights(build_plan(cfg)), device_id=0, precision=precision)

    stream = torch.cuda.Stream()
    gen = torch.Generator(device="cuda").manual_seed(20261018)

    def event_ms(eng, ids, out, group):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        L.check(eng.model.lib.jg_forward(eng.model.handle, ids.data_ptr(), L.JG_PTR_DEVICE, ids.shape[0], ids.shape[2],
                                         out.data_ptr(), None, None, None, L.JG_PTR_DEVICE, group, stream.cuda_stream), "jg_forward")
        e1.record(stream)
        stream.synchronize()
        return e0.elapsed_time(e1)

    few, many = 1, 5
    for fsize in (500, 2000):
        n_win = args.windows if fsize == 500 else max(args.windows // 4, 1)
        group = n_win                                   # one launch group: the whole batch
        for precision in ("f32",):
            legs = {n: engine(blocks(n), precision) for n in (few, many)}
            l = legs[few].model.row_length(fsize)
            hy = [x for x in legs[few].plan.rep if type(x).__name__ == "Hyena"][0]
            c, order = hy.channels, hy.order
            ids = torch.randint(1, 65, (n_win, 6, l), dtype=torch.uint8, device="cuda", generator=gen)
            out = torch.empty((n_win, legs[few].model.widths["prediction"]), dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()
            for eng in legs.values():                      # warm-up: workspace, code objects
                event_ms(eng, ids, out, group)
            ms = {n: [] for n in legs}
            for _ in range(args.repeats):                  # interleaved
                for n, eng in legs.items():
                    ms[n].append(event_ms(eng, ids, out, group))
            rows_l = l
            us = (float(np.median(ms[many])) - float(np.median(ms[few]))) * 1e3 / (many - few)
            flops = (legs[many].model.flops_per_window(l) - legs[few].model.flops_per_window(l)) / (many - few) * n_win
            floor_us = 2 * 4 * 6 * rows_l * c * n_win / (res["copy_rate_gbs"] * 1e9) * 1e6
            res[f"L{rows_l}"] = {
                "windows": n_win, "positions_per_frame": rows_l, "channels": c, "order": order, "launches_per_op": 2 + order,
                "us_per_op": round(us, 1), "us_per_launch": round(us / (2 + order), 1),
                "pass_ms": {f"{n} blocks": [round(v, 3) for v in ms[n]] for n in ms},
                "gflop_per_op": round(flops / 1e9, 2), "tflops": round(flops / (us * 1e-6) / 1e12, 2),
                "fraction_of_f32_vector_peak": round(flops / (us * 1e-6) / 1e12 / F32_VECTOR_PEAK_TFLOPS, 4),
                "hbm_floor_us": round(floor_us, 1), "multiple_of_hbm_floor": round(us / floor_us, 1)}
            for eng in legs.values():
                eng.close()
            del ids, out
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
