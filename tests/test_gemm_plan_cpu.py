"""The tile engine's launch planner (csrc/gemm_plan.h), checked without a GPU: in plan-only mode (lib.launch_log(3)) nk_gemm_dispatch logs the
plan of a call -- kernel, grid, block, LDS bytes, K split, accumulate mode, zero-fills, k rotation, patch height -- and returns before it
touches the device, so the entry points can be called with dummy pointers.

  * against the parent's record: tests/golden/tile_engine_plans.json holds what the commit before the planner launched for every case of
    tests/gemm_exact.py and every tile-engine call of the training step (printed at its launch sites); the planner must give the same line;
  * against the case table: the planned kernel of every case is the one the case expects (on the GPU: tests/test_gemm_exact_gpu.py);
  * the side queries (statistics-epilogue tiles, fused GEGLU forward, flipped input gradient) answer what the planner plans."""
import ctypes as C
import json
from pathlib import Path

import pytest

from neurosis_amd import lib
from tests import gemm_exact as G
from tests import gemm_plan_rows as R

FIXTURE = json.loads((Path(__file__).resolve().parent / "golden" / "tile_engine_plans.json").read_text())
ROWS = [(r[:4], r[4]) for r in FIXTURE["rows"]]
# colsum is no launch of the tile engine (nk_colsum has a kernel of its own): it has no plan
PLANNED_CASES = [c for c in G.CASES if c.op != "colsum"]


def test_fixture_covers_the_case_table_and_the_training_step():
    assert len(FIXTURE["parent"]) == 40 and FIXTURE["line"].split()[0] == "name"
    keys = {R.row_key(row) for row, _ in ROWS}
    assert len(keys) == len(ROWS) >= 300
    missing = [c.id for c in PLANNED_CASES if R.row_key(R.case_row(c)) not in keys]
    assert not missing, f"cases without a recorded plan: {missing}"
    ops = {row[0] for row, _ in ROWS}
    assert {"fwd", "fwd_geglu", "fwd_geglu_s", "fwd_batched", "dgrad", "dgrad_geglu", "dgrad_geglu_s", "wgrad", "wgrad_batched", "conv_fwd", "conv_dgrad",
            "conv_wgrad"} <= ops
    for op in ("wgrad", "wgrad_batched", "conv_wgrad"):       # each accumulate mode, with and without a bias gradient
        seen = {(row[2].get("accumulate"), bool(row[2].get("dbias"))) for row, _ in ROWS if row[0] == op and not row[3]}
        assert seen >= {(a, b) for a in (0, 1, 2) for b in (False, True)}, (op, seen)
    assert all(len(lines) == 1 and lines[0].count(" ") == 10 for _, lines in ROWS)


def test_plans_equal_the_parents_record():
    wrong = [(row, want, got) for row, want in ROWS if (got := R.plan_lines(lib, row)) != want]
    assert not wrong, f"{len(wrong)} of {len(ROWS)} plans differ from the record of {FIXTURE['parent'][:12]}; first (row, recorded, planned): {wrong[:3]}"


def test_planned_kernel_of_every_case_is_the_expected_one():
    wrong = [(c.id, c.expect, names) for c in PLANNED_CASES if (names := R.plan_names(lib, R.case_row(c))) != [c.expect]]
    assert not wrong, f"the dispatch moved (case, expected, planned): {wrong}"


def test_plan_only_mode_touches_no_device_and_logs_name_then_plan():
    c = G.BY_ID["wgrad-w160-split-by-shape-16384x5120x640"]      # a launch with a zero-fill in front: nothing of it may run here
    row = R.case_row(c)
    lib.launch_log(3)
    try:
        assert R.call_row(lib, row) == 0, "plan-only mode returns NK_OK without a device"
        log = lib.launched()
    finally:
        lib.launch_log(0)
    assert log[0] == c.expect and log[1].startswith(c.expect + " grid=") and len(log) == 2
    zero = int(log[1].split(" ")[7])
    assert zero == 3, "destination and bias gradient zero-filled first"
    with pytest.raises(lib.NkError):
        lib.launch_log(4)


def _conv_rows(op):
    return [row for row, _ in ROWS if row[0] == op and not row[3]]


def test_stats_tiles_query_is_the_plans_tiles_per_image():
    rows = _conv_rows("conv_fwd")
    assert rows
    halo = 0
    for row in rows:
        d = R._desc(row[1], row[2])
        tiles = lib.query("nk_conv2d_stats_tiles", C.byref(d), 0)
        line = R.plan_lines(lib, [row[0], row[1], {k: v for k, v in row[2].items() if k != "stats"}, row[3]])[0]
        is_halo = line.startswith("nk_conv3x3_halo_kernel<")
        assert (tiles > 0) == is_halo, (row, tiles, line)
        if is_halo:
            halo += 1
            bn = int(line.split("<")[1].split(",")[0])
            grid = int(line.split("grid=")[1].split(",")[0])
            N, Cout = row[1][0], row[1][4]
            assert grid == N * tiles * (Cout // bn), (row, tiles, line)
    assert 0 < halo < len(rows), "the rows must hold convolutions the halo kernel takes and ones it does not"


def test_geglu_query_is_the_planned_kernel():
    rows = [row for row, _ in ROWS if row[0] in ("fwd_geglu", "fwd_geglu_s")]
    shapes = {tuple(row[1]) for row in rows} | {(4096, 1280, 1280), (308, 640, 2048), (4096, 5120, 64)}     # and shapes the 256 x 256 kernel refuses
    answers = set()
    for M, I, K in sorted(shapes):
        ok = lib.query("nk_linear_fwd_geglu_ok", M, I, K)
        names = R.plan_names(lib, ["fwd_geglu", [M, I, K], {}, {}])
        assert (ok == 1) == (names == ["nk_gemm_xl2g_kernel<geglu=1>"]), (M, I, K, ok, names)
        assert ok or names == [], "a refused shape is an argument error, not another kernel"
        answers.add(ok)
    assert answers == {0, 1}


def test_flipped_dgrad_query_is_the_planned_kernel():
    rows = _conv_rows("conv_dgrad") + [["conv_dgrad", [4, 26, 26, 1280, 1280, 3, 1, 1], {}, {}], ["conv_dgrad", [2, 32, 32, 320, 320, 3, 2, 1], {}, {}]]
    answers = set()
    for row in rows:
        ok = lib.query("nk_conv2d_dgrad_flipped_ok", C.byref(R._desc(row[1], row[2])))
        names = R.plan_names(lib, [row[0], row[1], dict(row[2], flipped=1), row[3]])
        assert (ok == 1) == (len(names) == 1 and names[0].startswith("nk_conv3x3_halo_kernel<")), (row, ok, names)
        assert ok or names == [], "nk_conv2d_dgrad_flipped refuses what the query refuses"
        answers.add(ok)
    assert answers == {0, 1}
