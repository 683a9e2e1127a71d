"""The attention kernels (csrc/attention.hip, attn512.h, attn512_bwd.h, ops._attention_recompute_bwd) against float64 references computed
by torch on the GPU from the same bf16 inputs, on every dispatch path, at the training step's sizes and layouts: self-attention q / k / v
and dq / dk / dv are column slices of one [B L, 3 H D] buffer, cross-attention k / v slices of [B Lk, 2 H D] (modules/attention.py).
The case table, and the path each case takes, is tests/attention_bounds.py's (test_attention_bounds_cpu.py checks that it reaches every
branch of the dispatch).

Three kinds of check:
  exact   retrieval inputs: dense +-1 keys, values in {-1, 1}, dO in {-1, 0, 1}; query i = alpha k_a (one target) or alpha (k_a + k_b)
          (a tie), alpha a power of two, every target ahead of every other visible key by >= 120 natural units, so that every other
          weight underflows to exactly zero in fp32.  Every nonzero entry of a query has the same magnitude, so the d = 64 kernels round
          every entry of Q' alike: ties stay ties and margins stay margins.  O is then v_a or (v_a + v_b) / 2 bit for bit; with one
          target dS = 0 exactly, so dQ = 0 and dK gets nothing from that row; dV_j is the sum of the dO rows that target j; a tie gives
          dS_a = -dS_b = dO . (v_a - v_b) / 4.  dQ, dK, dV are held to the float64 sums within the relative error of the backward's P
          (fp32 rounding of scores and lse, ~16 u |lse|), one bf16 rounding of dS and half a bf16 ulp of the output: a misplaced key,
          row, split or head moves an output by O(1).  Targets cover every key of every (batch, head) where Lq >= Lk (first and last
          key of every tile included); causal rows pair a visible target with a masked key that scores as high.
  bounded Gaussian q, k at logit standard deviations 1, 4 and 8, per-row offsets up to +-60 natural units, rows whose maximum rises in
          the last key tile, dominant keys in the ragged last tile: every element of o, lse, dq, dk and dv against float64, within the
          first-order bound of attention_bounds.head_reference (its docstring lists each family's rounding points and the bound).
          Prints "[bound] ..." with the worst error / bound of every check.
  same    two runs are bit-identical, the second with the backward workspace NaN-filled (no kernel reads workspace it did not write,
          e.g. a query split that owns no tile) and the gradient slices NaN-filled (every gradient element is written).
"""
import math

import pytest
import torch

from tests import attention_bounds as ab

pytestmark = pytest.mark.gpu

F64 = torch.float64
BF16 = torch.bfloat16
U = ab.U


@pytest.fixture(scope="module")
def ops():
    from neurosis_amd import ops as o

    return o


@pytest.fixture(autouse=True)
def _free_memory():
    yield
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def _check(label, got, ref, bound):
    got = got.to(F64)
    assert torch.isfinite(got).all(), f"{label}: non-finite output"
    ratio = (got - ref).abs() / bound.clamp_min(1e-300)
    worst = float(ratio.max())
    print(f"[bound] {label}: worst error / bound = {worst:.3g}")
    if not worst <= 1.0:
        i = int(ratio.argmax())
        g, r, b = got.reshape(-1)[i], ref.reshape(-1)[i], bound.reshape(-1)[i]
        raise AssertionError(f"{label}: |got - ref| = {float((g - r).abs()):.4g} > bound {float(b):.4g} at flat index {i} "
                             f"(got {float(g):.8g}, ref {float(r):.8g}; worst error / bound {worst:.3g})")


def _exact(label, got, ref):
    got = got.to(F64)
    if not torch.equal(got, ref):
        bad = got != ref
        i = int(bad.reshape(-1).to(torch.int8).argmax())
        raise AssertionError(f"{label}: not bit-exact: {int(bad.sum())} of {got.numel()} differ, e.g. flat index {i}: "
                             f"got {float(got.reshape(-1)[i])}, ref {float(ref.reshape(-1)[i])}")
    print(f"[exact] {label}: bit-exact ({got.numel()} values)")


def _cid(c):
    return c[0]


# ================================================================================================================================
# running a case with the modules' layouts
# ================================================================================================================================
class Run:
    """q / k / v / dO token matrices in the case's layout, filled head by head; .go() calls the kernels"""

    def __init__(self, case):
        self.case = case
        _, self.env, B, H, Lq, Lk, D, self.causal, layout, self.bwd = case
        self.B, self.H, self.Lq, self.Lk, self.D = B, H, Lq, Lk, D
        HD = H * D
        dev = "cuda"
        if layout == "self":
            self.buf = torch.zeros(B * Lq, 3 * HD, dtype=BF16, device=dev)
            self.q, self.k, self.v = self.buf[:, :HD], self.buf[:, HD:2 * HD], self.buf[:, 2 * HD:]
        elif layout == "cross":
            self.q = torch.zeros(B * Lq, HD, dtype=BF16, device=dev)
            self.kv = torch.zeros(B * Lk, 2 * HD, dtype=BF16, device=dev)
            self.k, self.v = self.kv[:, :HD], self.kv[:, HD:]
        else:
            self.q = torch.zeros(B * Lq, HD, dtype=BF16, device=dev)
            self.k = torch.zeros(B * Lk, HD, dtype=BF16, device=dev)
            self.v = torch.zeros(B * Lk, HD, dtype=BF16, device=dev)
        self.layout = layout
        self.do = torch.zeros(B * Lq, HD, dtype=BF16, device=dev)

    def put(self, b, h, q, k, v, do):
        D = self.D
        self.q[b * self.Lq:(b + 1) * self.Lq, h * D:(h + 1) * D] = q
        self.k[b * self.Lk:(b + 1) * self.Lk, h * D:(h + 1) * D] = k
        self.v[b * self.Lk:(b + 1) * self.Lk, h * D:(h + 1) * D] = v
        self.do[b * self.Lq:(b + 1) * self.Lq, h * D:(h + 1) * D] = do

    def head(self, t, b, h, L):
        return t[b * L:(b + 1) * L, h * self.D:(h + 1) * self.D]

    def go(self, ops, monkeypatch, *, poison=False):
        for key, val in self.env.items():
            monkeypatch.setenv(key, val)
        if poison:
            monkeypatch.setattr(ops, "_ws", lambda n, device: torch.full((n,), float("nan"), dtype=torch.float32, device=device))
        B, H, D = self.B, self.H, self.D
        out = {}
        if self.bwd == "recompute":
            out["o"], bwd = ops.attention512_fwd(self.q, self.k, self.v, B)
            out["lse"] = None
            out["dq"], out["dk"], out["dv"] = bwd(self.do)
        else:
            need_lse = self.bwd is not None or D != 512
            o, bwd, lse = ops.attention_fwd(self.q, self.k, self.v, B, H, D, causal=self.causal, need_lse=need_lse, return_lse=True)
            out["o"], out["lse"] = o, lse
            if self.bwd:
                HD = H * D
                nan = float("nan")
                if self.layout == "self":
                    g = torch.full_like(self.buf, nan)
                    dq, dk, dv = g[:, :HD], g[:, HD:2 * HD], g[:, 2 * HD:]
                elif self.layout == "cross":
                    dq = torch.full_like(self.q, nan)
                    g = torch.full_like(self.kv, nan)
                    dk, dv = g[:, :HD], g[:, HD:]
                else:
                    dq, dk, dv = (torch.full_like(t, nan) for t in (self.q, self.k, self.v))
                bwd(self.do, dq, dk, dv)
                out["dq"], out["dk"], out["dv"] = dq, dk, dv
        torch.cuda.synchronize()
        if poison:
            monkeypatch.undo()
        return out


def _family(case):
    path = ab.case_path(case)
    return ab.family_of(path[1] or path[0]), path


# ================================================================================================================================
# exact: retrieval
# ================================================================================================================================
def _flips(n, D, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randint(0, 2, (n, D), generator=g, device="cuda").to(F64) * 2 - 1


def run_retrieval(ops, monkeypatch, case, two, seed=0):
    _, env, B, H, Lq, Lk, D, causal, layout, bwd = case
    fam, path = _family(case)
    label = f"{case[0]} {'tie' if two else 'one'} [{path[0]} / {path[1]}, qsplit {path[2]}]"
    scale = D ** -0.5
    k0, targets, alpha = ab.retrieval_base(Lq, Lk, D, two=two, causal=causal, seed=seed)
    ta, tb = targets[:, 0], targets[:, 1]
    tie = (tb >= 0) & (not causal)
    flips = _flips(B * H, D, seed + 7)
    g = torch.Generator(device="cuda").manual_seed(seed + 11)
    r = Run(case)
    heads = []
    for b in range(B):
        for h in range(H):
            k = k0 * flips[b * H + h]
            q = ab.retrieval_query(k, targets, alpha)
            v = torch.randint(0, 2, (Lk, D), generator=g, device="cuda").to(F64) * 2 - 1
            do = torch.randint(-1, 2, (Lq, D), generator=g, device="cuda").to(F64)
            r.put(b, h, q.to(BF16), k.to(BF16), v.to(BF16), do.to(BF16))
            heads.append((b, h, q, k, v, do))
    out = r.go(ops, monkeypatch)
    # the kernels' own target score: ln 2 Q'.k_a on the Q' paths (the same for every nonzero entry), scale q.k_a elsewhere
    c = torch.tensor(scale, dtype=torch.float32) * torch.tensor(ab.LOG2E, dtype=torch.float32)
    o_all, lse_all = [], []
    dq_ok = dk_ok = dv_ok = True
    for b, h, q, k, v, do in heads:
        o_ref = torch.where(tie[:, None], 0.5 * (v[ta] + v[tb.clamp_min(0)]), v[ta])
        o_all.append((r.head(out["o"], b, h, Lq), o_ref))
        qeff = ab.LN2 * (q.float() * c.cuda()).to(BF16).to(F64) if fam.qp_fwd else scale * q
        s_t = (qeff * k[ta]).sum(1)
        lse_ref = s_t + torch.where(tie, math.log(2.0), 0.0)
        if out["lse"] is not None:
            lse_all.append((out["lse"][b, h].to(F64), lse_ref, 16 * U * (lse_ref.abs() + 1)))
        if not bwd or fam.name in ("attn512", "recompute"):
            continue      # (the d = 512 backward rebuilds scores from the raw q against the forward's Q' lse: at these logits, hundreds of
            #              natural units, that is a relative shift of P of up to 2^-8 |logit|; the bounded checks cover it)
        eta = 16 * U * (lse_ref.abs() + 1)
        w = torch.where(tie, 0.5, 1.0).to(F64)
        n = (do * (v[ta] - v[tb.clamp_min(0)])).sum(1)
        dsa = torch.where(tie, 0.25 * n, torch.zeros_like(n))
        dds = torch.where(tie, 0.25 * n.abs() * (eta + ab.UB), torch.zeros_like(n))
        kb = k[tb.clamp_min(0)]
        dq_ref = scale * dsa[:, None] * (k[ta] - kb)
        dq_b = ab.SAFETY * scale * dds[:, None] * (k[ta].abs() + kb.abs())
        qk = qeff if fam.dk_qp else scale * q      # dK = ln 2 dS^T Q' on the attn64 paths
        dk_ref = torch.zeros(Lk, D, dtype=F64, device="cuda")
        dk_b = torch.zeros_like(dk_ref)
        dv_ref = torch.zeros_like(dk_ref)
        dv_b = torch.zeros_like(dk_ref)
        dk_ref.index_add_(0, ta, dsa[:, None] * qk)
        dk_b.index_add_(0, ta, dds[:, None] * qk.abs())
        dv_ref.index_add_(0, ta, w[:, None] * do)
        dv_b.index_add_(0, ta, (w * eta)[:, None] * do.abs())
        if bool(tie.any()):
            dk_ref.index_add_(0, tb[tie], -dsa[tie, None] * qk[tie])
            dk_b.index_add_(0, tb[tie], dds[tie, None] * qk[tie].abs())
            dv_ref.index_add_(0, tb[tie], 0.5 * do[tie])
            dv_b.index_add_(0, tb[tie], (0.5 * eta[tie])[:, None] * do[tie].abs())
        for name, got, ref, bnd in (("dq", r.head(out["dq"], b, h, Lq), dq_ref, dq_b), ("dk", r.head(out["dk"], b, h, Lk), dk_ref, dk_b),
                                    ("dv", r.head(out["dv"], b, h, Lk), dv_ref, dv_b)):
            bnd = ab.SAFETY * bnd if name != "dq" else bnd
            bnd = bnd + ab.half_ulp(ref, bnd)
            ratio = float(((got.to(F64) - ref).abs() / bnd.clamp_min(1e-300)).max()) if torch.isfinite(got).all() else math.inf
            if not ratio <= 1.0:
                _check(f"{label} {name} (batch {b}, head {h})", got, ref, bnd)
    _exact(f"{label} o ({B * H} heads)", torch.cat([g_ for g_, _ in o_all]), torch.cat([r_ for _, r_ in o_all]))
    if lse_all:
        _check(f"{label} lse ({B * H} heads)", torch.cat([a for a, _, _ in lse_all]), torch.cat([b_ for _, b_, _ in lse_all]),
               torch.cat([c_ for _, _, c_ in lse_all]))
    if bwd and fam.name not in ("attn512", "recompute"):
        print(f"[bound] {label} dq / dk / dv ({B * H} heads): every element within its bound")


@pytest.mark.parametrize("case", ab.REAL_CASES, ids=_cid)
def test_retrieval_real_sizes(ops, monkeypatch, case):
    run_retrieval(ops, monkeypatch, case, two=True, seed=1)
    if case[6] != 512 and case[3] * case[2] <= 40:
        run_retrieval(ops, monkeypatch, case, two=False, seed=2)


@pytest.mark.parametrize("case", ab.EDGE_CASES, ids=_cid)
def test_retrieval_edges(ops, monkeypatch, case):
    run_retrieval(ops, monkeypatch, case, two=case[4] % 2 == 1, seed=case[4] + case[5])


# ================================================================================================================================
# bounded: Gaussian inputs against float64
# ================================================================================================================================
def run_bounded(ops, monkeypatch, case, std, *, offsets=0.0, heads=None, seed=0):
    _, env, B, H, Lq, Lk, D, causal, layout, bwd = case
    fam, path = _family(case)
    label = f"{case[0]} std {std:g} off {offsets:g} [{path[0]} / {path[1]}, qsplit {path[2]}]"
    r = Run(case)
    data = {}
    for b in range(B):
        for h in range(H):
            q, k, v, do = ab.gaussian_head(Lq, Lk, D, std, offsets=offsets, late_max=True, tail_dominant=3,
                                           seed=seed + 97 * (b * H + h))
            r.put(b, h, q, k, v, do)
            data[(b, h)] = (q, k, v, do)
    out = r.go(ops, monkeypatch)
    for b, h in heads or [(0, 0), (B - 1, H - 1)]:
        q, k, v, do = data[(b, h)]
        ref = ab.head_reference(q, k, v, do if bwd else None, D ** -0.5, fam, causal=causal)
        _check(f"{label} o (b{b} h{h})", r.head(out["o"], b, h, Lq), *ref["o"])
        if out["lse"] is not None and fam.name != "recompute":
            _check(f"{label} lse (b{b} h{h})", out["lse"][b, h], *ref["lse"])
        if bwd:
            _check(f"{label} dq (b{b} h{h})", r.head(out["dq"], b, h, Lq), *ref["dq"])
            _check(f"{label} dk (b{b} h{h})", r.head(out["dk"], b, h, Lk), *ref["dk"])
            _check(f"{label} dv (b{b} h{h})", r.head(out["dv"], b, h, Lk), *ref["dv"])
    return out


_CASE = {c[0]: c for c in ab.REAL_CASES}
BOUNDED = [
    # (case, logit std, row offsets)
    ("sdxl-self-L4096", 1.0, 0.0), ("sdxl-self-L988", 8.0, 60.0), ("sdxl-self-L3952", 4.0, 60.0),
    ("sdxl-cross-L4096", 4.0, 60.0), ("sdxl-cross-L988", 8.0, 0.0),
    ("sdxl-cross-L3952-2k", 1.0, 60.0), ("sdxl-cross-L1024-2k", 8.0, 0.0),
    ("clip-l-causal", 4.0, 60.0), ("bigg-causal", 8.0, 0.0),
    ("sd15-cross-d40", 4.0, 60.0), ("sd15-self-d80", 1.0, 0.0), ("sd15-self-d160", 8.0, 60.0), ("sd15-cross-d80", 8.0, 0.0),
    ("generic64-self", 4.0, 60.0), ("generic64-cross", 1.0, 0.0),
    ("empty-split-small", 4.0, 0.0), ("empty-split-dkdv", 4.0, 0.0),
    ("vae-enc-L16384", 1.0, 0.0), ("vae-enc-L15808", 4.0, 0.0),
    ("vae-train-L1024", 1.0, 0.0), ("vae-train-L200", 4.0, 60.0), ("vae-recompute-L4096", 1.0, 0.0),
]


@pytest.mark.parametrize("name,std,offsets", BOUNDED, ids=[f"{n}-std{s:g}-off{o:g}" for n, s, o in BOUNDED])
def test_bounded_real_sizes(ops, monkeypatch, name, std, offsets):
    run_bounded(ops, monkeypatch, _CASE[name], std, offsets=offsets, seed=int(std) * 13 + int(offsets))


@pytest.mark.parametrize("Lq,Lk", [(1, 1), (33, 65), (129, 97), (31, 129), (129, 3)])
@pytest.mark.parametrize("variant", ["d64", "d64-2k", "d80", "d512"])
def test_bounded_edges(ops, monkeypatch, variant, Lq, Lk):
    D = {"d64": 64, "d64-2k": 64, "d80": 80, "d512": 512}[variant]
    env = ab.SMALL_OFF if variant == "d64-2k" else {}
    if D == 512:
        Lk = Lq
    case = (f"edge-{variant}-{Lq}x{Lk}", env, 3, 1 if D == 512 else 3, Lq, Lk, D, False, "dense" if D == 512 else "cross", True)
    run_bounded(ops, monkeypatch, case, 4.0, offsets=20.0, heads=[(0, 0), (2, case[3] - 1)], seed=Lq + Lk)


def test_qprime_term(ops, monkeypatch):
    """the Q' rounding of the d = 64 kernels at logit standard deviations 1, 4, 8: the d = 64 path and the generic kernels (NK_ATTN64=0)
    on the same inputs, each against float64, and the size of the Q' term E - Ebar (attention_bounds) against the rest of o's bound"""
    case = ("qprime", {}, 1, 2, 1024, 1024, 64, False, "self", True)
    for std in (1.0, 4.0, 8.0):
        errs = {}
        for name, env in (("attn64", {}), ("generic", ab.A64_OFF)):
            c = case[:1] + (env,) + case[2:]
            out = run_bounded(ops, monkeypatch, c, std, heads=[(0, 0)], seed=5)
            q, k, v, do = ab.gaussian_head(1024, 1024, 64, std, late_max=True, tail_dominant=3, seed=5)
            ref = ab.head_reference(q, k, v, do, 0.125, ab.FAMILIES["generic"])
            errs[name] = {n: float((Run(c).head(out[n], 0, 0, 1024).to(F64) - ref[n][0]).abs().max() / ref[n][0].abs().max())
                          for n in ("o", "dq", "dk", "dv")}
            monkeypatch.undo()
        print(f"[qprime] logit std {std:g}: max |err| / max |ref|  attn64 " + ", ".join(f"{n} {e:.2e}" for n, e in errs["attn64"].items())
              + "  generic " + ", ".join(f"{n} {e:.2e}" for n, e in errs["generic"].items()))


# ================================================================================================================================
# same: bit-identical repeats, poisoned workspace, NaN-filled gradients
# ================================================================================================================================
@pytest.mark.parametrize("name", ["empty-split-small", "empty-split-dkdv", "sd15-cross-d80", "sdxl-cross-L1024", "vae-train-L200"])
def test_repeat_poisoned_workspace(ops, monkeypatch, name):
    case = _CASE[name]
    _, env, B, H, Lq, Lk, D, causal, layout, bwd = case
    r = Run(case)
    for b in range(B):
        for h in range(H):
            r.put(b, h, *ab.gaussian_head(Lq, Lk, D, 4.0, seed=b * H + h))
    a = {n: t.clone() for n, t in r.go(ops, monkeypatch).items() if t is not None}
    monkeypatch.undo()
    z = r.go(ops, monkeypatch, poison=True)
    for n in a:
        assert torch.isfinite(z[n]).all(), f"{name}: {n} not finite with a NaN-filled workspace (a kernel read what it did not write)"
        assert torch.equal(a[n], z[n]), f"{name}: {n} differs between two runs on the same inputs"
    print(f"[same] {name}: bit-identical with a NaN-filled workspace and NaN-filled gradient slices")
