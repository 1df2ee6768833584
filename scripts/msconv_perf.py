#!/usr/bin/env python
"""Timing of the multi-scale conv op (csrc/jg_msconv.hip), for DESIGN.md 3.10 and profiles/msconv_perf.json.

The op has no profiling class of its own (JG_PROF_CLASSES is pinned), so it is timed from outside, by HIP events on a
stream handed to ``jg_forward``: embedding (C wide) -> ``multi_scale_conv`` (C -> C) -> batch norm -> gelu -> average pool ->
dense with ONE layer beside the same model with FIVE, device-resident ids and outputs, interleaved passes, one launch group -
the difference of the two event times over the four extra layers is one mask op and one conv op with the norm and the gelu
fused into its store.  For the fixture's layer (64 -> [16 k3 | 16 k5 | 32 k3 d3] -> 64) and the ``wide`` one of the tests
(128 -> [32 k15 | 32 k5 d16 | 48 k3 d2 relu | 16 k1] -> 128), at rows of 500-bp windows, in exact f32:

* microseconds per layer, and the achieved rate of its counted multiply-adds (``jg_model_flops_per_window``) beside the
  exact-f32 matrix peak - the nominal 157.3 TFLOP/s, and that figure scaled by the share of the nominal f16 rate which the
  box calibration (``jg_box_calibrate``, bench.py's ``box``) finds this device to hold under load;
* the yardstick: every branch as a ``masked_conv1d`` of its own (C -> filters, the branch's taps and dilation, the same norm
  and gelu) behind a one-tap front conv, the conv kernels' time from the engine's profiling classes (``mfma_f32`` /
  ``mfma_f16x3``) minus that of the model with the front conv alone - summed over the branches, in exact-f32 mode and in
  split-f16 mode.  Those models ran before this op existed; neither figure is the op compared with itself.

Usage: python scripts/msconv_perf.py [--windows 6144] [--repeats 5] [--out profiles/msconv_perf.json]
"""
import argparse
import copy
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

F32_MATRIX_PEAK_TFLOPS = 157.3
F16_MATRIX_PEAK_TFLOPS = 2500.0
LAYERS = {
    "fixture": (64, [dict(filters=16, kernel_size=3), dict(filters=16, kernel_size=5), dict(filters=32, kernel_size=3, dilation_rate=3)]),
    "wide": (128, [dict(filters=32, kernel_size=15), dict(filters=32, kernel_size=5, dilation_rate=16),
                   dict(filters=48, kernel_size=3, dilation_rate=2, activation="relu"), dict(filters=16, kernel_size=1)]),
}
NORM_ACT = [{"name": "masked_batchnorm", "config": {}}, {"name": "activation", "config": {"activation": "gelu"}}]


def model(c, hidden, out_c):
    import yaml
    cfg = yaml.safe_load((ROOT / "tests" / "golden" / "multiscale500_project.yaml").read_text())["model"]
    cfg["embedding"]["embedding_size"] = c
    cfg["representation_learner"]["hidden_layers"] = hidden
    cfg["classifier"]["input_shape"] = out_c
    return cfg


def stacked(c, branches, n):
    layer = {"name": "multi_scale_conv", "config": dict(branches=copy.deepcopy(branches), merge="concat")}
    return model(c, [x for _ in range(n) for x in [copy.deepcopy(layer)] + NORM_ACT], c)


def single(c, branch):
    front = [{"name": "masked_conv1d", "config": dict(filters=c, kernel_size=1, padding="same")}] + NORM_ACT
    if branch is None:
        return model(c, front, c)
    conv = dict(branch, padding="same")
    return model(c, front + [{"name": "masked_conv1d", "config": conv}] + NORM_ACT, branch["filters"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=6144)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    from jaeger_amd import _lib as L
    from jaeger_amd.engine import JaegerHipEngine
    from jaeger_amd.plan import build_plan
    from jaeger_amd.weights import random_weights

    def engine(cfg, precision):
        return JaegerHipEngine(model_cfg=cfg, weights=random_weights(build_plan(cfg)), device_id=0, precision=precision)

    stream = torch.cuda.Stream()
    gen = torch.Generator(device="cuda").manual_seed(20261019)

    def event_ms(eng, ids, out, group):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        L.check(eng.model.lib.jg_forward(eng.model.handle, ids.data_ptr(), L.JG_PTR_DEVICE, ids.shape[0], ids.shape[2],
                                         out.data_ptr(), None, None, None, L.JG_PTR_DEVICE, group, stream.cuda_stream), "jg_forward")
        e1.record(stream)
        stream.synchronize()
        return e0.elapsed_time(e1)

    def conv_kernel_ms(cfg, precision, ids, group):
        """Median over the repeats of the conv kernels' summed time in one forward (the engine's profiling classes)."""
        eng = engine(cfg, None)
        try:
            try:
                eng.model.set_precision(precision)
            except L.JaegerHipError:                   # (no split-f16 program for this model: nothing to report)
                return None
            out = torch.empty((ids.shape[0], eng.model.widths["prediction"]), dtype=torch.float32, device="cuda")
            event_ms(eng, ids, out, group)
            got = []
            for _ in range(args.repeats):
                eng.device.profile_enable(True)
                event_ms(eng, ids, out, group)
                p = eng.device.profile_read()
                eng.device.profile_enable(False)
                got.append(p["mfma_f32"]["ms"] + p["mfma_f16x3"]["ms"])
            return float(np.median(got))
        finally:
            eng.close()

    res = {"f32_matrix_peak_tflops": F32_MATRIX_PEAK_TFLOPS, "positions_per_workgroup": L.MSCONV_TILE, "windows": args.windows}
    few, many = 1, 5
    n_win = group = args.windows
    for name, (c, branches) in LAYERS.items():
        legs = {n: engine(stacked(c, branches, n), "f32") for n in (few, many)}
        l = legs[few].model.row_length(500)
        ids = torch.randint(1, 65, (n_win, 6, l), dtype=torch.uint8, device="cuda", generator=gen)
        out = torch.empty((n_win, legs[few].model.widths["prediction"]), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        for eng in legs.values():                      # warm-up: workspace, code objects
            event_ms(eng, ids, out, group)
        ms = {n: [] for n in legs}
        for _ in range(args.repeats):                  # interleaved
            for n, eng in legs.items():
                ms[n].append(event_ms(eng, ids, out, group))
        if "box" not in res:                           # straight behind timed work, on the chip as it left it
            res["box"] = legs[few].device.box_calibrate(0.5)
        us = (float(np.median(ms[many])) - float(np.median(ms[few]))) * 1e3 / (many - few)
        flops = (legs[many].model.flops_per_window(l) - legs[few].model.flops_per_window(l)) / (many - few) * n_win
        for eng in legs.values():
            eng.close()
        tflops = flops / (us * 1e-6) / 1e12
        held = F32_MATRIX_PEAK_TFLOPS * res["box"]["mfma_loop_tflops"] / F16_MATRIX_PEAK_TFLOPS
        row = {"channels_in": c, "channels_out": c, "positions_per_frame": l, "branches": branches,
               "us_per_layer": round(us, 1), "pass_ms": {f"{n} layers": [round(v, 3) for v in ms[n]] for n in ms},
               "gflop_per_layer": round(flops / 1e9, 2), "tflops": round(tflops, 2),
               "fraction_of_f32_matrix_peak": round(tflops / F32_MATRIX_PEAK_TFLOPS, 4),
               "f32_matrix_peak_at_the_box_rate_tflops": round(held, 1), "fraction_of_that": round(tflops / held, 4)}
        for precision in ("f32", "f16x3"):
            front = conv_kernel_ms(single(c, None), precision, ids, group)
            whole = [conv_kernel_ms(single(c, b), precision, ids, group) for b in branches]
            if front is None or None in whole:
                row[f"separate_convs_{precision}"] = None
                continue
            per_branch = [v - front for v in whole]
            row[f"separate_convs_{precision}"] = {"front_conv_us": round(front * 1e3, 1), "us_per_branch": [round(v * 1e3, 1) for v in per_branch],
                                                  "us_sum": round(sum(per_branch) * 1e3, 1),
                                                  "fused_op_over_sum": round(us / (sum(per_branch) * 1e3), 3)}
        res[name] = row
        del ids, out
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
