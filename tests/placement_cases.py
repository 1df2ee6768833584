"""Models and row lengths of the placement census (test_gpu_placement_census.py holds the engine to
golden/placement_census.json, which scripts/record_placement_census.py records): one model per family of DESIGN §0, each
at the window lengths that flip a placement - the small-window family at 500 bp (one fused launch) and at 755 bp (its first
conv's output beyond ``jg_small_max_positions()``: layer by layer), the two-strand model inside and beyond the table net's
160 KiB LDS bound (10 x 5 x 125 quads x 16 B + 16 KiB + the row: rows from about 47 400 bases on are out), the pyramid at
2 000 bp (window-packed tiles, phase-split tensors, fused residual blocks), and one model per row mixer (frame, local and
axial = frame + length attention, hyena behind a conv and as the first layer) at 500 bp, the smallest rows their fixtures
define.

What is recorded is decided on the host alone: launches and FLOPs per profiling class of one forward over 8 windows,
``describe()``, the placement statistics and the model's FLOPs per window (the only place the FLOP formulas of the ops
without a profiling class - length attention, hyena - are pinned).  None of it depends on what the kernels compute."""
import numpy as np

N_WIN = 8

#: model (op_cases.model_cfg names; dvf500 and the row-mixer models have weight generators of their own) -> window lengths in bases
MODELS = {
    "brain": (1500,),
    "zeus": (1500,),
    "pyramid": (2000,),
    "baseline500": (500, 755),
    "nmdmerge500": (500, 755),
    "dvf500": (500, 48000),
    "baseline500_dicodon_pos": (500,),
    "crossframe500": (500,),
    "localattn500": (500,),
    "axial500": (500,),
    "hyena500": (500,),
    "hyenafirst500": (500,),
    "brain_ln": (1500,),
}

#: row-mixer model -> the reference module whose random_weights its own GPU test uses
MIXER_REFERENCE = {
    "crossframe500": "attention_reference",
    "localattn500": "local_attention_reference",
    "axial500": "axial_attention_reference",
    "hyena500": "hyena_reference",
    "hyenafirst500": "hyena_reference",
}


def model_and_weights(name: str):
    import op_cases as oc
    from conftest import load_model_cfg
    if name == "dvf500":
        from oracle import strands as ost
        cfg = load_model_cfg(name)
        return cfg, ost.random_weights(cfg, seed=38341)
    if name in MIXER_REFERENCE:          # the weights each model's own GPU test uses
        import importlib
        cfg = load_model_cfg(name)
        return cfg, importlib.import_module(MIXER_REFERENCE[name]).random_weights(cfg)
    cfg = oc.model_cfg(name)
    return cfg, oc.weights_for(name, cfg)


def make_engine(name: str):
    import warnings

    from jaeger_amd.engine import JaegerHipEngine
    cfg, weights = model_and_weights(name)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")          # (the two-strand fixture's embedding.type note)
        return JaegerHipEngine(model_cfg=cfg, weights=weights, device_id=0)


def precisions(eng) -> tuple:
    """Both arithmetics where the model has both (a model starts in split-f16 mode when it is eligible)."""
    return ("f16x3", "f32") if eng.model.precision == "f16x3" else ("f32",)


def ids_for(eng, fsize: int, n_win: int = N_WIN, seed: int = 11) -> np.ndarray:
    rng = np.random.Generator(np.random.PCG64(seed))
    m = eng.model
    rows = m.strands if m.strands > 1 else 6
    vocab = 5 if m.strands > 1 else eng.program.vocab
    return rng.integers(0, vocab, (n_win, rows, m.row_length(fsize))).astype(np.uint16 if m.wide_ids else np.uint8)


def census(name: str) -> dict:
    """{"describe", "stats", "flops_per_window": {"<fsize>": flops}, "runs": {"<fsize> <precision>": {class: [launches, flops]}}}
    of one model."""
    eng = make_engine(name)
    try:
        out = {"describe": eng.model.describe(), "stats": eng.model.placement(), "runs": {},
               "flops_per_window": {str(fsize): eng.model.flops_per_window(eng.model.row_length(fsize)) for fsize in MODELS[name]}}
        for prec in precisions(eng):
            eng.model.set_precision(prec)
            for fsize in MODELS[name]:
                ids = ids_for(eng, fsize)
                eng.device.profile_enable(True)
                eng.model.forward(ids, want=("prediction",))
                prof = eng.device.profile_read()
                eng.device.profile_enable(False)
                assert eng.model.precision == prec, (name, fsize, prec, "the f16 range guard tripped")
                out["runs"][f"{fsize} {prec}"] = {k: [v["launches"], v["flops"]] for k, v in prof.items() if isinstance(v, dict)}
        return out
    finally:
        eng.close()
