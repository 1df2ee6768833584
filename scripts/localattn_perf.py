#!/usr/bin/env python
"""Timing of the local-attention kernel (csrc/jg_localattn.hip), for DESIGN.md 3.6 and profiles/localattn_perf.json.

No parent commit ran such a model, so the yardstick is the frame-attention op (csrc/jg_frameattn.hip) on the same box in
the same session: the localattn500 model (tests/golden, one block here) beside crossframe500 - the same channels, heads,
feed-forward width, row length and windows per launch -, in interleaved passes, both ops timed by the HIP events of
jg_profile_enable:

* microseconds per launch, the fraction of the exact-f32 matrix-core peak its dense products reach (halo included), the
  multiple of the HBM floor (2 x 4 B x 6 L C per window over the device-to-device copy rate of the same run);
* the ratio to the frame-attention launch per token, beside the ratio the dense-FLOP counts predict:
  [(2 C^2 + 2 C F) + 2 C^2 (T + 2 halo) / T] / (4 C^2 + 2 C F).

Usage: python scripts/localattn_perf.py [--windows 12288] [--repeats 5] [--out profiles/localattn_perf.json]
"""
import argparse
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "scripts"))

from frameattn_perf import F32_MFMA_PEAK_TFLOPS, copy_rate_gbs  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=12288)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import yaml

    from jaeger_amd import _lib as L
    from jaeger_amd.engine import JaegerHipEngine
    from jaeger_amd.plan import LocalAttn, build_plan
    from jaeger_amd.weights import random_weights
    fsize, n_win = 500, args.windows
    rng = np.random.Generator(np.random.PCG64(20261017))
    seq = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, fsize * n_win)].copy()
    starts = (np.arange(n_win) * fsize).astype(np.int64)
    lens = np.full(n_win, fsize, np.int32)
    res = {"windows": n_win, "fsize": fsize, "copy_rate_gbs": round(copy_rate_gbs(), 1)}

    def engine(name, precision, **over):
        cfg = yaml.safe_load((ROOT / "tests" / "golden" / f"{name}_project.yaml").read_text())["model"]
        for layer in cfg["representation_learner"]["hidden_layers"]:
            if layer["name"] == "local_attention":
                layer["config"].update(over)
        plan = build_plan(cfg)
        return JaegerHipEngine(model_cfg=cfg, weights=random_weights(plan), device_id=0, precision=precision), plan

    want = ("prediction",)
    for precision in ("f32", "f16x3"):
        legs = {"local": engine("localattn500", precision, num_blocks=1), "frame": engine("crossframe500", precision)}
        for eng, _ in legs.values():                   # warm-up: workspace, code objects
            eng.predict_windows(seq, starts, lens, fsize, want=want)
        acc = {k: {"ms": 0.0, "launches": 0, "flops": 0.0, "cvt_ms": 0.0, "cvt_launches": 0} for k in legs}
        for _ in range(args.repeats):                  # interleaved
            for k, (eng, _) in legs.items():
                eng.device.profile_enable(True)
                eng.predict_windows(seq, starts, lens, fsize, want=want)
                prof = eng.device.profile_read_local_attn() if k == "local" else eng.device.profile_read()
                eng.device.profile_enable(False)
                op, cvt = (prof["local_attn"], prof["local_attn_cvt"]) if k == "local" else (prof["frame_attn"], prof["frame_attn_cvt"])
                for key in ("ms", "launches", "flops"):
                    acc[k][key] += op[key]
                acc[k]["cvt_ms"] += cvt["ms"]
                acc[k]["cvt_launches"] += cvt["launches"]
        eng, plan = legs["local"]
        layer = [x for x in plan.rep if isinstance(x, LocalAttn)][0]
        c, f, h = layer.channels, layer.ff_dim, layer.half_window
        l = eng.model.row_length(fsize)
        t, halo = L.LOCALATTN_TILE, (h + 15) // 16 * 16
        row = {}
        for k, a in acc.items():
            us = a["ms"] * 1e3 / a["launches"]
            win_per_launch = n_win * args.repeats / a["launches"]
            floor_us = 2 * 4 * 6 * l * c * win_per_launch / (res["copy_rate_gbs"] * 1e9) * 1e6
            row[k] = {"us_per_launch": round(us, 1), "windows_per_launch": win_per_launch, "positions_per_frame": l,
                      "dense_tflops": round(a["flops"] / (a["ms"] * 1e-3) / 1e12, 2),
                      "fraction_of_f32_mfma_peak": round(a["flops"] / (a["ms"] * 1e-3) / 1e12 / F32_MFMA_PEAK_TFLOPS, 3),
                      "hbm_floor_us": round(floor_us, 1), "multiple_of_hbm_floor": round(us / floor_us, 1),
                      "f16s_to_f32_conversion_us_per_launch": round(a["cvt_ms"] * 1e3 / a["cvt_launches"], 1) if a["cvt_launches"] else None}
        per_token = {k: acc[k]["ms"] / acc[k]["launches"] / row[k]["windows_per_launch"] for k in acc}
        expected = ((2 * c * c + 2 * c * f) + 2 * c * c * (t + 2 * halo) / t) / (4 * c * c + 2 * c * f)
        res[precision] = {"local attention, one block": row["local"], "frame attention": row["frame"],
                          "channels": c, "feed_forward": f, "half_window": h, "tile": t, "halo": halo,
                          "ratio_to_frame_attention_per_token": round(per_token["local"] / per_token["frame"], 3),
                          "ratio_expected_from_dense_flops": round(expected, 3),
                          "band_flops_per_position": 4 * (2 * h + 1) * c}
        for e, _ in legs.values():
            e.close()
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
