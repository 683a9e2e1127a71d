"""The attention dispatch on the GPU against its own plan (csrc/attn_plan.h), one small descriptor per path:
  * a real call launches, under lib.launch_log(1), the kernels the plan-only mode names for it, in order;
  * the backward stays inside the workspace nk_attention_bwd_ws_floats reports: the floats behind it keep their bit pattern, and the
    gradients equal, bit for bit, those of a run with a generously oversized workspace (a wrong offset would write inside the allocation
    and move them)."""
import ctypes as C

import pytest
import torch

from neurosis_amd import lib
from tests import attention_bounds as ab
from tests import attn_plan_rows as R

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16

A64_OFF = {"NK_ATTN64": "0"}
FWD64, FWDG, RED = "attn64_fwd_kernel", "attn_fwd_kernel", "attn_dkv_reduce_kernel"
GEN = ["attn_bwd_dq_kernel", "attn_bwd_dkdv_kernel"]
# (id, env, [B, H, Lq, Lk, D, causal], backward pass, the kernels of forward + backward, query splits, last split empty)
# 33 query tiles at Lq = 1040: the one-kernel backward splits them 16 ways, the dK / dV kernels 8 ways (5 tiles each: the last split has none)
PATHS = [
    ("small-16-splits", {}, [1, 2, 1040, 77, 64, 0], "bwd", [FWD64, "attn64_bwd_small_kernel", RED], 16, True),
    ("dq-dkdv-splits", {}, [1, 2, 1040, 120, 64, 0], "bwd", [FWD64, "attn64_bwd_dq_kernel", "attn64_bwd_dkdv_kernel", RED], 8, True),
    ("dq-dkdv", {}, [1, 2, 129, 129, 64, 0], "bwd", [FWD64, "attn64_bwd_dq_kernel", "attn64_bwd_dkdv_kernel"], 1, False),
    ("generic-dp96-splits", {}, [1, 2, 1040, 77, 80, 0], "bwd", [FWDG] + GEN + [RED], 8, True),
    ("generic-dp64-attn64-off", A64_OFF, [1, 2, 33, 65, 64, 0], "bwd", [FWDG] + GEN, 1, False),
    ("generic-dp64-d40", {}, [1, 2, 33, 65, 40, 0], "bwd", [FWDG] + GEN, 1, False),
    ("generic-dp160", {}, [1, 2, 33, 65, 160, 0], "bwd", [FWDG] + GEN, 1, False),
    ("causal", {}, [1, 2, 77, 77, 64, 1], "bwd_causal", [FWD64, "attn64_bwd_small_kernel<causal>"], 1, False),
    ("d512", {}, [1, 1, 33, 33, 512, 0], "bwd", ["attn512_fwd_kernel", "attn512_delta_kernel", "attn512_bwd_kernel<0>", "attn512_bwd_kernel<1>"], 0, False),
]
DP_SMEM = {"generic-dp96-splits": 96, "generic-dp64-attn64-off": 64, "generic-dp64-d40": 64, "generic-dp160": 160}


@pytest.fixture(scope="module")
def ops():
    from neurosis_amd import ops as o

    return o


def _inputs(dims, seed=0):
    B, H, Lq, Lk, D, _ = dims
    g = torch.Generator(device="cuda").manual_seed(seed)
    mk = lambda L: (torch.randn(B * L, H * D, generator=g, device="cuda") * 0.7).to(BF16)
    return mk(Lq), mk(Lk), mk(Lk), mk(Lq)


@pytest.mark.parametrize("case", PATHS, ids=[p[0] for p in PATHS])
def test_dispatch_launches_what_it_plans(ops, monkeypatch, case):
    cid, env, dims, bwd_pass, names, qsplit, empty = case
    B, H, Lq, Lk, D, causal = dims
    fwd, bwd = R.planned(lib, dims, env, "fwd"), R.planned(lib, dims, env, bwd_pass)
    planned = [l["name"] for l in fwd["launches"] + bwd["launches"]]
    assert planned == names and bwd["qsplit"] == qsplit and ab.empty_split(Lq, max(qsplit, 1)) == empty, (planned, bwd)
    if cid in DP_SMEM:
        assert {ab._generic_dp(l) for l in (fwd["launches"] + bwd["launches"])[:2]} == {DP_SMEM[cid]}      # forward and dQ: the query-block ring
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    q, k, v, do = _inputs(dims)
    lib.launch_log(1)
    try:
        if causal:
            _, b_att = ops.attention_causal_fwd(q, k, v, B, H, D)
        else:
            _, b_att = ops.attention_fwd(q, k, v, B, H, D)
        b_att(do)
        launched = lib.launched()
    finally:
        lib.launch_log(0)
    torch.cuda.synchronize()
    assert launched == planned


PATTERN = 0x5AA55AA5
TAIL = 4096


@pytest.mark.parametrize("case", [p for p in PATHS if p[3] == "bwd"], ids=[p[0] for p in PATHS if p[3] == "bwd"])
def test_backward_stays_inside_the_planned_workspace(ops, monkeypatch, case):
    _, env, dims, _, _, _, _ = case
    B, H, Lq, Lk, D, _ = dims
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    q, k, v, do = _inputs(dims, seed=1)
    o, _, lse = ops.attention_fwd(q, k, v, B, H, D, return_lse=True)
    d = R.desc(dims)
    n = lib.query("nk_attention_bwd_ws_floats", C.byref(d))
    assert n == R.planned(lib, dims, env, "bwd")["ws"]

    def run(ws):
        ws.view(torch.int32).fill_(PATTERN)
        grads = [torch.full_like(t, float("nan")) for t in (q, k, v)]
        lib.call("nk_attention_bwd", C.byref(d), q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), lse.data_ptr(), do.data_ptr(),
                 *[g.data_ptr() for g in grads], ws.data_ptr(), ops._stream())
        torch.cuda.synchronize()
        return grads

    tight = torch.empty(n + TAIL, dtype=torch.float32, device="cuda")
    got = run(tight)
    tail = tight.view(torch.int32)[n:]
    assert tail.numel() == TAIL and bool((tail == PATTERN).all()), f"{int((tail != PATTERN).sum())} floats behind the workspace were written"
    want = run(torch.empty(2 * n + (1 << 20), dtype=torch.float32, device="cuda"))
    for name, a, b in zip(("dq", "dk", "dv"), got, want):
        assert not bool(torch.isnan(a.float()).any()), name
        assert torch.equal(a.view(torch.int16), b.view(torch.int16)), f"{name} moves with the size of the workspace"
