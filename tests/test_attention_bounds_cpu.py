"""The attention error bounds of tests/attention_bounds.py against a torch emulation of each kernel family's rounding points (CPU):
the emulated arithmetic stays inside the bounds, and each planted fault leaves them.  Also: the GPU test's case table, mapped through the
plan nk_attention_fwd / nk_attention_bwd make for each case (plan-only mode: no GPU), reaches every kernel path."""
import pytest
import torch

from tests import attention_bounds as ab

F64 = torch.float64


def _worst(emu, ref, names):
    worst = {}
    for n in names:
        r, b = ref[n]
        worst[n] = float(((emu[n].to(F64) - r).abs() / b.clamp_min(1e-300)).max())
    return worst


SHAPES = [(100, 130, 64), (64, 77, 64), (33, 65, 80), (40, 40, 40)]


@pytest.mark.parametrize("fam", ["attn64", "generic", "attn512", "recompute"])
@pytest.mark.parametrize("std,offsets", [(1.0, 0.0), (4.0, 60.0), (8.0, 20.0)])
def test_emulation_inside_bounds(fam, std, offsets):
    f = ab.FAMILIES[fam]
    for i, (Lq, Lk, D) in enumerate(SHAPES):
        q, k, v, do = ab.gaussian_head(Lq, Lk, D, std, offsets=offsets, late_max=True, tail_dominant=3, seed=i, device="cpu")
        ref = ab.head_reference(q, k, v, do, D ** -0.5, f)
        emu = ab.emulate(q, k, v, do, f, qsplit=4)
        worst = _worst(emu, ref, ("o", "lse", "dq", "dk", "dv"))
        print(f"[bound] emulated {fam} {Lq}x{Lk} d{D} std {std:g} offsets {offsets:g}: " + ", ".join(f"{n} {w:.3g}" for n, w in worst.items()))
        assert max(worst.values()) <= 1.0, worst
        # not vacuous: the modelled roundings reach a fair share of every bound
        assert min(worst[n] for n in ("o", "dq", "dk", "dv")) >= 0.05, worst


def test_emulation_causal_inside_bounds():
    q, k, v, _ = ab.gaussian_head(77, 77, 64, 4.0, seed=3, device="cpu")
    ref = ab.head_reference(q, k, v, None, 0.125, ab.FAMILIES["attn64"], causal=True)
    worst = _worst(ab.emulate(q, k, v, None, ab.FAMILIES["attn64"], causal=True), ref, ("o", "lse"))
    print(f"[bound] emulated causal attn64 77x77: {worst}")
    assert max(worst.values()) <= 1.0


def _truncation_inputs():
    """one key at the row maximum (p = 1, exact) and 64 at p = 0.50388: just below the bf16 value 0.50391, so truncation loses almost a
    whole spacing (2^-8 / 0.504 relative) where rounding loses 0.00006 relative; every value 1.9375, so o = 1.9375 exactly"""
    D, Lq, Lk = 64, 4, 65
    q = torch.zeros(Lq, D)
    q[:, 0], q[:, 1] = 5.46875, 0.01469
    k = torch.zeros(Lk, D)
    k[1:, :2] = -1.0
    v = torch.full((Lk, D), 1.9375)
    return q.to(ab.BF16), k.to(ab.BF16), v.to(ab.BF16), None


FAULTS = [
    # (fault, family, inputs, what must leave its bound)
    ("drop_tail_key", "attn64", dict(logit_std=1.0, tail_dominant=2), "o"),
    ("drop_tail_key", "generic", dict(logit_std=1.0, tail_dominant=2), "o"),
    ("lse_neighbour", "attn64", dict(logit_std=4.0, offsets=20.0), "dv"),
    ("lse_neighbour", "generic", dict(logit_std=4.0, offsets=20.0), "dq"),
    ("lse_neighbour", "recompute", dict(logit_std=4.0, offsets=20.0), "dv"),
    ("split_missing", "attn64", dict(logit_std=1.0), "dv"),
    ("split_missing", "generic", dict(logit_std=1.0), "dk"),
    ("truncate_p", "generic", None, "o"),
]


@pytest.mark.parametrize("fault,fam,inputs,out", FAULTS, ids=[f"{f[0]}-{f[1]}" for f in FAULTS])
def test_planted_fault_leaves_bound(fault, fam, inputs, out):
    f = ab.FAMILIES[fam]
    if inputs is None:
        q, k, v, do = _truncation_inputs()
    else:
        q, k, v, do = ab.gaussian_head(256, 130, 64, seed=5, device="cpu", **inputs)
    ref = ab.head_reference(q, k, v, do, q.shape[1] ** -0.5, f)
    clean = _worst(ab.emulate(q, k, v, do, f, qsplit=4), ref, [out])[out]
    bad = _worst(ab.emulate(q, k, v, do, f, qsplit=4, fault=fault), ref, [out])[out]
    print(f"[bound] fault {fault} ({fam}): {out} worst error / bound {bad:.3g} (without the fault {clean:.3g})")
    assert clean <= 1.0
    assert bad > 1.0, f"{fault}: the bound of {out} does not catch it ({bad:.3g})"


REQUIRED = {
    "fwd": {"attn64_fwd", "attn64_fwd_causal", "generic_fwd_dp64", "generic_fwd_dp96", "generic_fwd_dp160", "attn512_fwd", "attn512_fwd_nolse"},
    "bwd": {"attn64_small", "attn64_small_qsplit", "attn64_dq_dkdv", "attn64_dq_dkdv_qsplit", "generic_bwd_dp64", "generic_bwd_dp64_qsplit",
            "generic_bwd_dp96", "generic_bwd_dp96_qsplit", "generic_bwd_dp160", "attn512_flash", "attn512_recompute"},
}


def test_case_table_reaches_every_path():
    paths = [ab.case_path(c) for c in ab.REAL_CASES + ab.EDGE_CASES]
    fwd = {p[0] for p in paths}
    bwd = {p[1] for p in paths if p[1]}
    assert REQUIRED["fwd"] <= fwd, REQUIRED["fwd"] - fwd
    assert REQUIRED["bwd"] <= bwd, REQUIRED["bwd"] - bwd
    # empty query splits on both split kernels, whole tiles and ragged tails of the d = 64 forward, every query-split count in use
    empty = {p[1] for p in paths if p[4]}
    assert {"attn64_small_qsplit", "attn64_dq_dkdv_qsplit"} <= empty, empty
    assert any(p[0] == "attn64_fwd" and p[3] and c[5] % 64 for p, c in zip(paths, ab.REAL_CASES + ab.EDGE_CASES))
    assert {p[2] for p in paths if p[1] and p[1].startswith("attn64_small")} >= {1, 4, 8}
    assert {p[2] for p in paths if p[1] and p[1].startswith(("attn64_dq", "generic"))} >= {1, 4, 8, 16}
    real = {c[0]: ab.case_path(c) for c in ab.REAL_CASES}
    assert [real[f"sdxl-cross-L{L}"][2] for L in (4096, 1024, 3952, 988)] == [8, 4, 8, 4]
    assert [real[f"sdxl-cross-L{L}-2k"][2] for L in (4096, 1024, 3952, 988)] == [16, 8, 16, 4]
    assert [real[f"sd15-cross-d{d}"][2] for d in (40, 80, 160)] == [16, 8, 1]
