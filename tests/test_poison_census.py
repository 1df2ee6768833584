"""CPU tier of tests/test_gpu_poison.py: every ``__global__`` kernel of jaeger_amd/csrc is either launched by a named case of
tests/poison_cases.py or carries one sentence on why it reads no grow-only workspace.  A kernel added later fails here until it is
given one or the other; a name that left the sources, or a case name the module no longer produces, fails as well."""
import poison_cases as pc


def test_every_kernel_is_mapped_and_every_mapping_is_live():
    found = pc.source_kernels()
    assert len(found) >= 40, sorted(found)                    # (the parser still finds the kernels)
    for probe in ("conv_f16x3_kernel", "conv_f32_kernel", "conv_pc_kernel", "small_net_kernel", "nmd_final_kernel"):
        assert probe in found, probe                           # (a name on the line behind its attributes, a template, a plain one)
    unmapped = sorted(set(found) - set(pc.KERNELS))
    assert not unmapped, f"kernels without a poison case or a reason (tests/poison_cases.py KERNELS): {unmapped}"
    gone = sorted(set(pc.KERNELS) - set(found))
    assert not gone, f"KERNELS names kernels the sources no longer hold: {gone}"
    names = set(pc.ALL_NAMES)
    assert len(names) == len(pc.ALL_NAMES)
    for kernel, entry in pc.KERNELS.items():
        if isinstance(entry, str):
            assert entry.strip().endswith(".") and len(entry.split()) >= 6, (kernel, entry)
            continue
        assert entry, f"{kernel}: no case launches it"
        dead = sorted(set(entry) - names)
        assert not dead, f"{kernel}: mapped to cases poison_cases does not produce: {dead}"
    print("\nkernels: %d in the sources, %d launched by cases, %d with a reason; cases per family: %s" % (
        len(found), sum(1 for e in pc.KERNELS.values() if not isinstance(e, str)),
        sum(1 for e in pc.KERNELS.values() if isinstance(e, str)), pc.families()))


def test_the_case_list_holds_every_source_case():
    import conv_instance_cases as cc
    import f32_conv_cases as fc32
    import fused_cases as fu
    import head_cases as hc
    import resblock_cases as rc
    names = set(pc.ALL_NAMES)
    assert {"conv/" + c.name for c in cc.CASES} <= names
    assert {"f32conv/" + c.name for c in fc32.CASES} | {"f32ln/" + c.name for c in fc32.LN_CASES} <= names
    assert {("resblock-guard/" if c.guard else "resblock/") + c.name for c in rc.CASES} <= names
    assert {"small/" + n for n in fu.SMALL_VARIANTS} <= names
    assert {f"tab/{n}-{form}" for n in fu.TAB_VARIANTS for form in ("mfma", "lds")} <= names
    assert {f"head/dense-{n}-{b}" for n in hc.DENSE_FAMILIES for b in ("bias", "nobias")} <= names
    for mx in pc.MIXERS:
        variants = pc.mixer_variants(mx)
        assert len(variants) >= 8, (mx.key, variants)
        assert {f"mixer/{mx.key}-{v}-{p}" for v in variants for p in ("own", "f32")} <= names
    assert {"history/" + f for f in ("brain", "pyramid", "baseline500", "dvf500", "legacy", "mixer_chain")} <= names
    # every dense kernel in one launch group of 13 windows, and the plain one in groups of 5, 5 and 3
    assert {hc.dense_kernel(hc.ROWS, cin, cout) for cin, cout in hc.DENSE_WANT} == {"tiled", "narrow", "plain"}
    assert all(hc.dense_kernel(n, cin, cout) != "tiled" for n in hc.groups_of(hc.ROWS, hc.CHUNK) for cin, cout in hc.DENSE_WANT)
