#!/usr/bin/env python
"""Timing of the bilstm op (csrc/jg_bilstm.hip), for DESIGN.md 3.9 and profiles/bilstm_perf.json.

The op has no profiling class of its own (JG_PROF_CLASSES is pinned), so it is timed from outside, by HIP events on a
stream handed to ``jg_forward``: embedding (64 wide) -> ``masked_bilstm`` -> batch norm -> average pool -> dense with ONE
layer beside the same model with FIVE, device-resident ids and outputs, interleaved passes, one launch group - the
difference of the two event times over the four extra ops is one op.  The extra layers read what a layer of ``units``
leaves, so the op timed has C = 2 x units incoming channels.  Per row length (166 positions: 500-bp windows; 665: 2 000-bp
windows) and for units 32 and 64, in exact f32 (the only conv of the model is the one-tap identity conv in front of the first
layer):

* microseconds per op;
* the achieved rate of the counted multiply-adds (``jg_model_flops_per_window``: x W and h R of both directions; the
  element-wise work is not counted) beside the 157.3 TFLOP/s f32 matrix peak;
* the multiple of the HBM floor: one read of the (6, L, C) and one write of the (6, L, 2U) f32 rows per window over the
  device-to-device copy rate measured first.

Usage: python scripts/bilstm_perf.py [--windows 6144] [--repeats 5] [--out profiles/bilstm_perf.json]
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

F32_MATRIX_PEAK_TFLOPS = 157.3


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
    res = {"copy_rate_gbs": round(copy_rate_gbs(), 1), "f32_matrix_peak_tflops": round(F32_MATRIX_PEAK_TFLOPS, 1),
           "rows_per_workgroup": L.BILSTM_ROWS, "steps_per_time_block": L.BILSTM_STEPS}
    base = yaml.safe_load((ROOT / "tests" / "golden" / "bilstm500_project.yaml").read_text())["model"]

    def layers(n, units):
        """The fixture's embedding, n bilstm layers of `units`, its closing batch norm, pool and head."""
        cfg = copy.deepcopy(base)
        rep = cfg["representation_learner"]["hidden_layers"]
        lstm = [l for l in rep if l["name"] == "masked_bilstm"][0]
        lstm["config"]["units"] = units
        cfg["representation_learner"]["hidden_layers"] = [copy.deepcopy(lstm) for _ in range(n)] + [rep[-1]]
        cfg["classifier"]["input_shape"] = 2 * units
        return cfg

    def engine(cfg):
        return JaegerHipEngine(model_cfg=cfg, weights=random_weights(build_plan(cfg)), device_id=0, precision="f32")

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

    few, many = 1, 5
    for fsize in (500, 2000):
        n_win = args.windows if fsize == 500 else max(args.windows // 4, 1)
        group = n_win                                   # one launch group: the whole batch
        for units in (32, 64):
            legs = {n: engine(layers(n, units)) for n in (few, many)}
            l = legs[few].model.row_length(fsize)
            c = 2 * units
            ids = torch.randint(1, 65, (n_win, 6, l), dtype=torch.uint8, device="cuda", generator=gen)
            out = torch.empty((n_win, legs[few].model.widths["prediction"]), dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()
            for eng in legs.values():                      # warm-up: workspace, code objects
                event_ms(eng, ids, out, group)
            ms = {n: [] for n in legs}
            for _ in range(args.repeats):                  # interleaved
                for n, eng in legs.items():
                    ms[n].append(event_ms(eng, ids, out, group))
            us = (float(np.median(ms[many])) - float(np.median(ms[few]))) * 1e3 / (many - few)
            flops = (legs[many].model.flops_per_window(l) - legs[few].model.flops_per_window(l)) / (many - few) * n_win
            floor_us = 4 * 6 * l * (c + 2 * units) * n_win / (res["copy_rate_gbs"] * 1e9) * 1e6
            groups = 2 * -(-6 * n_win // L.BILSTM_ROWS)
            res[f"L{l}_U{units}"] = {
                "windows": n_win, "positions_per_frame": l, "channels_in": c, "units": units, "workgroups": groups,
                "us_per_op": round(us, 1), "pass_ms": {f"{n} layers": [round(v, 3) for v in ms[n]] for n in ms},
                "gflop_per_op": round(flops / 1e9, 2), "tflops": round(flops / (us * 1e-6) / 1e12, 2),
                "fraction_of_f32_matrix_peak": round(flops / (us * 1e-6) / 1e12 / F32_MATRIX_PEAK_TFLOPS, 4),
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
