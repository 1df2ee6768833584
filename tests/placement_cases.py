"""Models and row lengths of the placement census (test_gpu_placement_census.py holds the engine to
golden/placement_census.json, which scripts/record_placement_census.py records): one model per family of DESIGN §0, each
at the window lengths that flip a placement - the small-window family at 500 bp (one fused launch) and at 755 bp (its first
conv's output beyond ``jg_small_max_positions()``: layer by layer), the two-strand model inside and beyond the table net's
160 KiB LDS bound (10 x 5 x 125 quads x 16 B + 16 KiB + the row: rows from about 47 400 bases on are out), the pyramid at
2 000 bp (window-packed tiles, phase-split tensors, fused residual blocks).

What is recorded is decided on the host alone: launches and FLOPs per profiling class of one forward over 8 windows,
``describe()`` and the placement statistics.  None of it depends on what the kernels compute."""
import numpy as np

N_WIN = 8

#: model (op_cases.model_cfg names; dvf500 and crossframe500 have weight generators of their own) -> window lengths in bases
MODELS = {
    "brain": (1500,),
    "zeus": (1500,),
    "pyramid": (2000,),
    "baseline500": (500, 755),
    "nmdmerge500": (500, 755),
    "dvf500": (500, 48000),
    "baseline500_dicodon_pos": (500,),
    "crossframe500": (500,),
    "brain_ln": (1500,),
}


def model_and_weights(name: str):
    import op_cases as oc
    from conftest import load_model_cfg
    if name == "dvf500":
        from oracle import strands as ost
        cfg = load_model_cfg(name)
        return cfg, ost.random_weights(cfg, seed=38341)
    if name == "crossframe500":
        import attention_reference as ar
        cfg = load_model_cfg(name)
        return cfg, ar.random_weights(cfg)
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
    """{"describe", "stats", "runs": {"<fsize> <precision>": {class: [launches, flops]}}} of one model."""
    eng = make_engine(name)
    try:
        out = {"describe": eng.model.describe(), "stats": eng.model.placement(), "runs": {}}
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
