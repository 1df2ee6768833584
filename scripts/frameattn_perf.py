#!/usr/bin/env python
"""Timing of the frame-attention kernel (csrc/jg_frameattn.hip) on the crossframe500 model, for the DESIGN.md row and
profiles/frameattn_perf.json:

* microseconds per attention launch at the default launch group (HIP events around the launch: jg_profile_enable),
  the fraction of the exact-f32 matrix-core peak its dense products reach, and the multiple of the HBM floor
  (2 x 4 B x 6 L C per window over the device-to-device copy rate measured on the same box in the same run);
* the cost of the F16S -> f32 layout conversion the split-f16 program queues in front of the op (a launch of its own,
  timed by its own pair of events: what a kernel variant that loads F16S directly would save);
* end-to-end Mbp/s (encode + forward, device-resident result rows copied back) of crossframe500 beside baseline500, in
  interleaved runs: baseline500 as shipped (the fused small-window kernel) and layer by layer (precision f32: the fused
  kernel is a split-f16 kernel).

Usage: python scripts/frameattn_perf.py [--windows 12288] [--repeats 5] [--out profiles/frameattn_perf.json]
"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

F32_MFMA_PEAK_TFLOPS = 157.3      # v_mfma_f32_16x16x4_f32 / 32x32x2, MI355X data sheet


def copy_rate_gbs() -> float:
    """Device-to-device copy rate (bytes read + bytes written per second) of a 1 GiB tensor, best of 5, by HIP events."""
    import torch
    n = 1 << 28
    a = torch.empty(n, dtype=torch.float32, device="cuda")
    b = torch.empty_like(a)
    best = 0.0
    for _ in range(6):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        b.copy_(a)
        t1.record()
        torch.cuda.synchronize()
        best = max(best, 2 * 4 * n / (t0.elapsed_time(t1) * 1e-3) / 1e9)
    del a, b
    torch.cuda.empty_cache()
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=12288)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import yaml

    from jaeger_amd.engine import JaegerHipEngine
    from jaeger_amd.plan import build_plan, frame_attn_flops_per_position
    from jaeger_amd.weights import random_weights
    fsize, n_win = 500, args.windows
    rng = np.random.Generator(np.random.PCG64(20261017))
    seq = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, fsize * n_win)].copy()
    starts = (np.arange(n_win) * fsize).astype(np.int64)
    lens = np.full(n_win, fsize, np.int32)
    res = {"windows": n_win, "fsize": fsize, "copy_rate_gbs": round(copy_rate_gbs(), 1)}

    def engine(name, precision):
        cfg = yaml.safe_load((ROOT / "tests" / "golden" / f"{name}_project.yaml").read_text())["model"]
        plan = build_plan(cfg)
        return JaegerHipEngine(model_cfg=cfg, weights=random_weights(plan), device_id=0, precision=precision), plan

    legs = {"crossframe500 f16x3": engine("crossframe500", "f16x3"), "crossframe500 f32": engine("crossframe500", "f32"),
            "baseline500 f16x3 (fused small-window kernel)": engine("baseline500", "f16x3"),
            "baseline500 f32 (layer by layer)": engine("baseline500", "f32")}
    want = ("prediction",)
    for eng, _ in legs.values():                       # warm-up: workspace, code objects
        eng.predict_windows(seq, starts, lens, fsize, want=want)
    times = {k: [] for k in legs}
    for _ in range(args.repeats):                      # interleaved
        for k, (eng, _) in legs.items():
            t0 = time.perf_counter()
            eng.predict_windows(seq, starts, lens, fsize, want=want)
            times[k].append(time.perf_counter() - t0)
    res["end_to_end_mbps"] = {k: {"median": round(n_win * fsize / float(np.median(v)) / 1e6, 1),
                                  "runs": [round(n_win * fsize / t / 1e6, 1) for t in v]} for k, v in times.items()}
    # the attention launch by HIP events
    for k in ("crossframe500 f16x3", "crossframe500 f32"):
        eng, plan = legs[k]
        l = eng.model.row_length(fsize)
        eng.device.profile_enable(True)
        for _ in range(args.repeats):
            eng.predict_windows(seq, starts, lens, fsize, want=want)
        prof = eng.device.profile_read()
        eng.device.profile_enable(False)
        fa = prof["frame_attn"]
        groups = fa["launches"] / args.repeats
        us = fa["ms"] * 1e3 / fa["launches"]
        win_per_launch = n_win / groups
        name, dense, core = frame_attn_flops_per_position(plan)[0]
        c = [x for x in plan.rep if type(x).__name__ == "FrameAttn"][0].channels
        floor_us = 2 * 4 * 6 * l * c * win_per_launch / (res["copy_rate_gbs"] * 1e9) * 1e6
        res[f"attention launch, {k}"] = {
            "us_per_launch": round(us, 1), "windows_per_launch": win_per_launch, "positions_per_frame": l,
            "dense_tflops": round(fa["flops"] / (fa["ms"] * 1e-3) / 1e12, 2),
            "fraction_of_f32_mfma_peak": round(fa["flops"] / (fa["ms"] * 1e-3) / 1e12 / F32_MFMA_PEAK_TFLOPS, 3),
            "hbm_floor_us": round(floor_us, 1), "multiple_of_hbm_floor": round(us / floor_us, 1),
            "all_kernels_event_ms_per_pass": round(prof["conv_ms"] / args.repeats, 3),
            "attention_event_ms_per_pass": round(fa["ms"] / args.repeats, 3),
            "f16s_to_f32_conversion_us_per_launch": (round(prof["frame_attn_cvt"]["ms"] * 1e3 / prof["frame_attn_cvt"]["launches"], 1)
                                                     if prof["frame_attn_cvt"]["launches"] else None),
            "flops_per_position": {"dense": dense, "scores_softmax_context": core}}
    for eng, _ in legs.values():
        eng.close()
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
