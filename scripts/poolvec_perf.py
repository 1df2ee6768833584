#!/usr/bin/env python
"""Timing of the pool-and-merge op (csrc/jg_poolvec.hip), for DESIGN.md 3.12 and profiles/poolvec_perf.json.

1. The op against the yardstick, ``pool_kernel`` (JG_OP_POOL, as it was before this op existed), on the same tensor.  Neither op
   has a profiling class, so both are timed from outside, by HIP events on a stream handed to ``jg_forward``, device-resident
   ids and outputs, one launch group, exact f32 (no pool is fused into a conv's store there).  Three models share the trunk
   embedding 16 -> one-tap conv -> C channels:

   * ``pool``  - ``pooling: max`` (or average): the trunk and ONE JG_OP_POOL;
   * ``one``   - ``parallel_branches`` of ONE branch without layers: the trunk and ONE JG_OP_POOLVEC (STORE) on the same tensor;
   * ``four``  - four such branches, concat: the trunk and FOUR of them.

   Interleaved passes; from the medians ``poolvec = (four - one) / 3`` and ``pool = pool_pass - one + poolvec``.  Shapes:
   6 x 165 x 32 and 6 x 500 x 128 per window, 4096 windows.  Each op reads its tensor once: the bytes over the time is the
   achieved read rate.
2. ``--forwards N``: N forwards of the fixture model (tests/golden/branches500_project.yaml) and nothing else - the run a
   kernel trace is taken of (``rocprofv3 --kernel-trace --stats --output-format csv -- python scripts/poolvec_perf.py --forwards 20``);
   ``--fold-stats CSV``: that trace's per-kernel table, folded into the JSON as the model's per-op time split.

Usage: python scripts/poolvec_perf.py [--windows 4096] [--repeats 9] [--out profiles/poolvec_perf.json]
"""
import argparse
import copy
import csv
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

SHAPES = {"6x165x32": (165, 32), "6x500x128": (500, 128)}


def fixture():
    import yaml
    return yaml.safe_load((ROOT / "tests" / "golden" / "branches500_project.yaml").read_text())["model"]


def model(c, pooling, n_branches):
    cfg = fixture()
    cfg["embedding"]["embedding_size"] = 16
    trunk = [{"name": "masked_conv1d", "config": dict(filters=c, kernel_size=1, padding="same")}]
    rep = cfg["representation_learner"]
    if n_branches == 0:
        rep["hidden_layers"], rep["pooling"] = trunk, pooling
        cfg["classifier"]["input_shape"] = c
    else:
        branch = {"hidden_layers": [], "pooling": pooling}
        rep["hidden_layers"] = trunk + [{"name": "parallel_branches",
                                         "config": {"merge": "concat", "branches": [copy.deepcopy(branch) for _ in range(n_branches)]}}]
        rep["pooling"] = None
        cfg["classifier"]["input_shape"] = c * n_branches
    return cfg


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=4096)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--forwards", type=int, default=0)
    ap.add_argument("--fold-stats", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    if args.fold_stats:                                    # no GPU: the trace's table into the JSON
        rows = [r for r in csv.DictReader(open(args.fold_stats))            # the model's own kernels: not the runtime's copies and fills, not torch's id generator
                if not r.get("Name", "").startswith("__amd_rocclr") and "at::native" not in r.get("Name", "")]
        key = lambda row, *names: next(row[n] for n in names if n in row)
        total = sum(float(key(r, "TotalDurationNs", "TotalDuration")) for r in rows)
        split = [{"kernel": key(r, "Name", "KernelName"), "calls": int(key(r, "Calls")),
                  "us_per_call": round(float(key(r, "TotalDurationNs", "TotalDuration")) / int(key(r, "Calls")) / 1e3, 2),
                  "share": round(float(key(r, "TotalDurationNs", "TotalDuration")) / total, 4)} for r in rows]
        out = Path(args.out)
        res = json.loads(out.read_text()) if out.exists() else {}
        res["fixture_kernel_split"] = {"windows": args.windows, "precision": "the model's default (split-f16 convs)",
                                       "kernels": sorted(split, key=lambda r: -r["share"])}
        out.write_text(json.dumps(res, indent=1) + "\n")
        print(json.dumps(res["fixture_kernel_split"], indent=1))
        return

    import torch

    from jaeger_amd import _lib as L
    from jaeger_amd.engine import JaegerHipEngine
    from jaeger_amd.plan import build_plan
    from jaeger_amd.weights import random_weights

    trunk = {}                                             # the legs of one comparison share the trunk's weights

    def engine(cfg, precision):
        weights = random_weights(build_plan(cfg))
        for k in weights:
            if not k.startswith("classifier/"):
                weights[k] = trunk.setdefault(k, weights[k])
        return JaegerHipEngine(model_cfg=cfg, weights=weights, device_id=0, precision=precision)

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

    n_win = group = args.windows
    if args.forwards:
        eng = engine(fixture(), None)
        ids = torch.randint(1, 65, (n_win, 6, eng.model.row_length(500)), dtype=torch.uint8, device="cuda", generator=gen)
        out = torch.empty((n_win, eng.model.widths["prediction"]), dtype=torch.float32, device="cuda")
        ms = [event_ms(eng, ids, out, group) for _ in range(args.forwards)]
        print(json.dumps({"fixture_forward_ms": [round(v, 3) for v in ms]}))
        eng.close()
        return

    res = {"windows": n_win, "precision": "f32", "method": "HIP events around jg_forward, interleaved passes, medians; "
           "poolvec = (four - one) / 3, pool = pool_pass - one + poolvec"}
    for shape, (l, c) in SHAPES.items():
        for pooling in ("max", "average"):
            trunk.clear()
            legs = {"pool": engine(model(c, pooling, 0), "f32"), "one": engine(model(c, pooling, 1), "f32"),
                    "four": engine(model(c, pooling, 4), "f32")}
            ids = torch.randint(1, 65, (n_win, 6, l), dtype=torch.uint8, device="cuda", generator=gen)
            ids[:, :, l - l // 8:] = 0                     # trailing padding: the masked path of both kernels
            outs = {k: torch.empty((n_win, e.model.widths["prediction"]), dtype=torch.float32, device="cuda") for k, e in legs.items()}
            embs = {}
            for k, e in legs.items():                      # warm-up, and the results must not differ: same sums, same order
                event_ms(e, ids, outs[k], group)
                embs[k] = e.model.forward(ids[:64].cpu().numpy())["embedding"]
            same = bool(np.array_equal(embs["pool"], embs["one"]) and np.array_equal(embs["four"][:, :c], embs["one"]))
            ms = {k: [] for k in legs}
            for _ in range(args.repeats):
                for k, e in legs.items():
                    ms[k].append(event_ms(e, ids, outs[k], group))
            med = {k: float(np.median(v)) for k, v in ms.items()}
            pv = (med["four"] - med["one"]) / 3.0
            pool = med["pool"] - med["one"] + pv
            gb = n_win * 6 * l * (c * 4 + 1) / 1e9
            res[f"{shape} {pooling}"] = {
                "pass_ms": {k: [round(x, 3) for x in v] for k, v in ms.items()},
                "pass_spread_ms": {k: round(float(np.max(v) - np.min(v)), 3) for k, v in ms.items()},
                "poolvec_us": round(pv * 1e3, 1), "pool_kernel_us": round(pool * 1e3, 1),
                "poolvec_over_pool_kernel": round(pv / pool, 3) if pool > 0 else None,
                "gb_read_per_op": round(gb, 3), "poolvec_gb_per_s": round(gb / (pv * 1e-3), 0) if pv > 0 else None,
                "pool_kernel_gb_per_s": round(gb / (pool * 1e-3), 0) if pool > 0 else None,
                "embedding_bit_identical_to_pool_kernel": same}
            for e in legs.values():
                e.close()
            del ids, outs
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
