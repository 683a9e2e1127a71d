"""The attention kernels' launch planner (csrc/attn_plan.h), checked without a GPU: in plan-only mode (lib.launch_log(3)) nk_attention_fwd,
nk_attention_bwd and nk_attention_bwd_causal log the plan of a call -- per launch the kernel, grid, block, LDS bytes and gx, and the query
splits, the offset of their partials and the workspace size -- and return before they touch the device or a pointer.

  * against the parent's record: tests/golden/attention_plans.json holds what the commit before the planner launched for every case of
    tests/attention_bounds.py, every attention call of the training step and the NK_ATTN_XCD=0 form of every path (printed at its launch
    sites); the planner must plan the same, and nk_attention_bwd_ws_floats must report the same size;
  * the layout fits the workspace it reports."""
import ctypes as C
import json
from pathlib import Path

import pytest

from neurosis_amd import lib
from tests import attention_bounds as ab
from tests import attn_plan_rows as R
from tests.test_attention_bounds_cpu import REQUIRED

FIXTURE = json.loads((Path(__file__).resolve().parent / "golden" / "attention_plans.json").read_text())
ROWS = [(r[:4], r[4]) for r in FIXTURE["rows"]]
KERNELS = {"attn64_fwd_kernel", "attn_fwd_kernel", "attn512_fwd_kernel", "attn64_bwd_small_kernel", "attn64_bwd_small_kernel<causal>",
           "attn64_bwd_dq_kernel", "attn64_bwd_dkdv_kernel", "attn_bwd_dq_kernel", "attn_bwd_dkdv_kernel", "attn_dkv_reduce_kernel",
           "attn512_delta_kernel", "attn512_bwd_kernel<0>", "attn512_bwd_kernel<1>"}


def test_fixture_covers_the_case_table_and_the_training_step():
    assert len(FIXTURE["parent"]) == 40 and FIXTURE["line"] == "name grid=x,y,z block smem gx qsplit part_offset ws_floats"
    assert [row for row, _ in ROWS] == R.rows(), "the fixture's rows are attn_plan_rows.rows(): the case table, the step, the 3-D grids"
    keys = {(row[0], json.dumps(row[2], sort_keys=True)) for row, _ in ROWS}
    assert len(keys) == len(ROWS) >= len(ab.REAL_CASES + ab.EDGE_CASES) + 25
    assert all(set(row[3]) == set(rec) - {"ws_floats"} for row, rec in ROWS)
    launches = [(row, pass_, l) for row, rec in ROWS for pass_ in row[3] for l in rec[pass_]["launches"]]
    assert {l["name"] for _, _, l in launches} == KERNELS
    # every path the bounds test requires (the chunked recompute beyond ops.ATTN512_FLASH_MAX_L tokens is no attention launch)
    paths = [ab.case_path(c) for c in ab.REAL_CASES + ab.EDGE_CASES]
    assert REQUIRED["fwd"] <= {p[0] for p in paths} and REQUIRED["bwd"] <= {p[1] for p in paths if p[1]}
    # both grid forms of every kernel that has them, and the three generic instances by their LDS bytes
    for name in KERNELS - {"attn_dkv_reduce_kernel", "attn512_delta_kernel", "attn512_bwd_kernel<0>", "attn512_bwd_kernel<1>"}:
        assert {l["gx"] > 0 for _, _, l in launches if l["name"] == name} == {True, False}, name
    assert {l["smem"] for _, _, l in launches if l["name"] == "attn_bwd_dq_kernel"} == {256 * (2 * dp + 16) for dp in (64, 96, 160)}
    for row, _, l in launches:
        B, H = row[1][:2]
        assert l["grid"] == ([l["gx"] * H * B, 1, 1] if l["gx"] else l["extent"]) and (not l["gx"] or l["extent"] == [l["gx"], H, B]), (row, l)


def test_plans_equal_the_parents_record():
    wrong = []
    for row, rec in ROWS:
        for pass_ in row[3]:
            got = R.planned(lib, row[1], row[2], pass_)
            want = dict(rec[pass_], ws=rec["ws_floats"] if pass_ == "bwd" else 0)
            if got != want:
                wrong.append((row, pass_, want, got))
    assert not wrong, f"{len(wrong)} plans differ from the record of {FIXTURE['parent'][:12]}; first (row, pass, recorded, planned): {wrong[:2]}"


def test_ws_floats_equal_the_parents_record():
    wrong = [(row, rec["ws_floats"], got) for row, rec in ROWS if (got := lib.query("nk_attention_bwd_ws_floats", C.byref(R.desc(row[1])))) != rec["ws_floats"]]
    assert not wrong, wrong[:3]
    with R.environment({"NK_ATTN64": "0", "NK_ATTN64_SMALL": "0"}):      # the size does not move with the switches
        assert all(lib.query("nk_attention_bwd_ws_floats", C.byref(R.desc(row[1]))) == rec["ws_floats"] for row, rec in ROWS)


def test_layout_fits_the_workspace():
    seen = 0
    for row, rec in ROWS:
        if "bwd" not in row[3]:
            continue
        B, H, Lq, Lk, D, _ = row[1]
        plan = R.planned(lib, row[1], row[2], "bwd")
        total = plan["ws"]
        assert total == rec["ws_floats"]
        rows = B * H * Lq
        # what sits in front of the partials: -delta, -lse2 (a padded row count each) and Q' [rows][64] bf16 on the head-dim-64 kernels, delta elsewhere
        names = {l["name"] for l in plan["launches"]}
        front = 2 * (-(-rows // 64) * 64) + rows * 32 if names & {"attn64_bwd_small_kernel", "attn64_bwd_dq_kernel"} else rows
        assert front <= total, (row, front, total)
        if plan["qsplit"] > 1:
            seen += 1
            assert plan["part"] % 4 == 0 and front <= plan["part"], (row, plan)
            assert plan["part"] + plan["qsplit"] * 2 * B * Lk * H * D <= total, (row, plan)
        else:
            assert plan["part"] == -1
    assert seen >= 12


def test_plan_only_mode_touches_no_pointer_and_logs_name_then_plan():
    dims = [2, 20, 1040, 120, 64, 0]          # dQ, dK / dV over 8 splits, reduce
    lib.launch_log(3)
    try:
        assert R.call(lib, dims, "bwd", None) == 0, "plan-only mode returns NK_OK with null pointers, without a device"
        log = lib.launched()
    finally:
        lib.launch_log(0)
    assert log[0::2] == ["attn64_bwd_dq_kernel", "attn64_bwd_dkdv_kernel", "attn_dkv_reduce_kernel"]
    assert all(line.startswith(name + " grid=") and line.count(" ") == 7 for name, line in zip(log[0::2], log[1::2])) and len(log) == 6
    assert [int(line.split(" ")[5]) for line in log[1::2]] == [8, 8, 8]
    # a descriptor the path refuses is refused in plan-only mode too, and the switches are read per call
    assert R.planned(lib, [1, 2, 77, 64, 64, 1], {}, "fwd") is None and R.planned(lib, [1, 2, 77, 77, 64, 0], {}, "bwd_causal") is None
    assert R.planned(lib, [1, 2, 33, 65, 64, 0], {"NK_ATTN64": "0"}, "fwd")["launches"][0]["name"] == "attn_fwd_kernel"
    assert R.planned(lib, [1, 2, 33, 65, 64, 0], {}, "fwd")["launches"][0]["name"] == "attn64_fwd_kernel"
    with pytest.raises(lib.NkError):
        lib.call("nk_attention_fwd", C.byref(R.desc(dims)), None, None, None, None, None, None)      # outside plan-only mode null pointers are an argument error
