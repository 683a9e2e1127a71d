"""The launch planner of the normalisation and column-sum kernels (csrc/norm_plan.h), checked without a GPU: in plan-only mode
(lib.launch_log(3)) the nk_groupnorm_*, nk_layernorm_*, nk_rmsnorm_fwd, nk_colsum* and nk_colpart_reduce_batch entry points log the plan of
a call -- per launch the kernel, grid, block, LDS bytes, the workspace regions it touches and the workspace size -- and return before they
touch the device or a pointer.

  * against the parent's record: tests/golden/norm_plans.json holds what the commit before the planner launched, and where in the
    workspace, for every row of tests/norm_plan_rows.py (printed at its launch sites); the planner must plan the same, and the size
    queries must report the same;
  * the layout fits the workspace the queries report, and the regions of one call do not overlap."""
import json
from pathlib import Path

from neurosis_amd import lib
from tests import norm_plan_rows as R

FIXTURE = json.loads((Path(__file__).resolve().parent / "golden" / "norm_plans.json").read_text())
ROWS = R.fixture_rows(FIXTURE)
KERNELS = {"gn_stats_kernel", "gn_reduce_partials_kernel", "gn_reduce_partials_l1_kernel", "gn_apply_kernel", "gn_apply_kernel<mod>",
           "gn_bwd_stats_kernel", "gn_bwd_stats_kernel<mod>", "colpart_reduce_kernel", "colpart_reduce_mod_kernel", "gn_dmod_kernel",
           "gn_bwd_apply_kernel", "gn_bwd_apply_kernel<mod>", "ln_fwd_kernel", "rms_fwd_kernel", "ln_bwd_dx_kernel", "ln_bwd_param_kernel",
           "ln_bwd_rows_kernel", "colpart_reduce_batch_kernel", "colsum_partial", "colsum_reduce"}


def _launches(entry=None):
    return [(row, R.parse(l)) for row, rec in ROWS if entry is None or row[0] == entry for l in rec["lines"]]


def test_fixture_covers_every_row_and_every_edge():
    assert len(FIXTURE["parent"]) == 40 and FIXTURE["line"] == "name grid=x,y,z block smem [region=offset+extent ...] ws=ws_floats"
    assert [row for row, _ in ROWS] == R.rows(), "the fixture's rows are norm_plan_rows.rows(), all of them, in order"
    assert {row[0] for row, _ in ROWS} == set(R.ENTRIES) and {l["name"] for _, l in _launches()} == KERNELS
    # one and two channel slabs; rows_per clamped at 32 (a short image in one block) and not
    assert {l["grid"][2] for _, l in _launches("gn_bwd") if l["name"] == "gn_bwd_stats_kernel"} == {1, 2}
    stats = {tuple(row[1]): l["grid"][0] for row, l in _launches("gn_fwd") if l["name"] == "gn_stats_kernel"}
    assert stats[(3, 63, 640, 32)] == 2 and stats[(1, 33, 8, 1)] == 2 and stats[(1, 1048576, 128, 32)] == 1024
    # one and two levels of the sums from partial rows, on both sides of the threshold
    levels = {row[1][1]: len(rec["lines"]) for row, rec in ROWS if row[0] == "gn_sums_from_parts"}
    assert levels[128] == 1 and levels[129] == 2 and levels[1] == 1 and levels[4096] == 2
    # every chunks-per-lane instance of LayerNorm (2, 3, 4) and RMSNorm (2, 4, 8), on both sides of each threshold
    assert {1024, 1032, 1536, 1544, 2048} <= {row[1][1] for row, _ in ROWS if row[0] == "ln_bwd_rows"}
    assert {1024, 1032, 2048, 2056, 4096} <= {row[1][1] for row, _ in ROWS if row[0] == "rms_fwd"}
    # widths only nk_layernorm_bwd_params takes: its partial rows must fit what nk_layernorm_ws_floats reports (test_regions_fit... checks)
    assert {2056, 4096} <= {row[1][1] for row, _ in ROWS if row[0] == "ln_bwd_params"}
    # column sums: 64 rows per block up to 65 536 rows, more beyond; the batched form; one and NK_COLPART_MAX entries
    split = {row[1][0]: l["grid"][0] for row, l in _launches("colsum") if l["name"] == "colsum_partial"}
    assert split[65536] == 1024 and split[65537] == 513 and split[2097152] == 1024
    assert {row[1][2] for row, _ in ROWS if row[0] == "colsum_batched"} >= {2, 3, 4}
    assert {len(row[1][0]) for row, _ in ROWS if row[0] == "colpart_batch"} == {1, 3, lib.NK_COLPART_MAX}


def test_plans_equal_the_parents_record():
    wrong = [(row, rec["lines"], got) for row, rec in ROWS if (got := R.plan_lines(lib, row)) != rec["lines"]]
    assert not wrong, f"{len(wrong)} plans differ from the record of {FIXTURE['parent'][:12]}; first (row, recorded, planned): {wrong[:2]}"


def test_size_queries_equal_the_parents_record_and_the_plan():
    for row, rec in ROWS:
        q = R.queries(lib, row)
        assert q == {k: v for k, v in rec.items() if k != "lines"}, (row, q)
        lines = [R.parse(l) for l in R.plan_lines(lib, row)]
        assert len({l["ws"] for l in lines}) == 1
        if row[0] in ("ln_bwd_rows", "ln_bwd"):
            assert lines[0]["regions"]["part"] == (0, q["part_rows"] * 2 * row[1][1])
        if row[0] == "ln_bwd_rows":      # the caller's `part` buffer: exactly nk_layernorm_part_rows(M) rows
            assert lines[0]["ws"] == q["part_rows"] * 2 * row[1][1]
        elif "ws" in q and row[0] not in ("ln_fwd", "ln_bwd_dx"):      # (the two LayerNorm passes without a workspace report 0)
            assert lines[0]["ws"] == q["ws"] * (row[1][2] if row[0] == "colsum_batched" else 1), (row, lines[0], q)
        else:
            assert lines[0]["ws"] == 0


def test_regions_fit_the_workspace_and_do_not_overlap():
    seen = 0
    for row, _ in ROWS:
        regions = {}
        for l in (R.parse(s) for s in R.plan_lines(lib, row)):
            for name, (off, n) in l["regions"].items():
                assert off >= 0 and n > 0 and off + n <= l["ws"], (row, l)
                assert regions.setdefault(name, (off, n)) == (off, n), (row, name)
        spans = sorted(regions.values())
        assert all(a[0] + a[1] <= b[0] for a, b in zip(spans, spans[1:])), (row, regions)
        seen += len(spans) > 1
    assert seen >= 100      # the GroupNorm forward (part | gsum) and backward (part | gsum | chan) of every shape


def test_plan_only_mode_touches_no_pointer_and_logs_name_then_plan():
    row = ["gn_mod_bwd", [2, 1024, 2560, 32]]
    lib.launch_log(3)
    try:
        assert R.call_row(lib, row) == 0, "plan-only mode returns NK_OK with null pointers, without a device"
        log = lib.launched()
    finally:
        lib.launch_log(0)
    assert log[0::2] == ["gn_bwd_stats_kernel<mod>", "gn_reduce_partials_kernel", "colpart_reduce_mod_kernel", "gn_dmod_kernel", "gn_bwd_apply_kernel<mod>"]
    assert all(line.startswith(name + " grid=") for name, line in zip(log[0::2], log[1::2])) and len(log) == 10
    # a shape the family refuses is refused in plan-only mode too ...
    for bad in (["gn_fwd", [1, 64, 12, 1]], ["gn_bwd", [1, 64, 64, 3]], ["gn_fwd", [1, 64, 4104, 1]], ["gn_apply", [1, 64, 520, 65]],
                ["gn_sums_from_parts", [1, 4, 33]], ["ln_fwd", [4, 2056]], ["ln_bwd_rows", [4, 12]], ["rms_fwd", [4, 4104]],
                ["colsum", [4, 12, 1]], ["colpart_batch", [[8] * 33, 4]], ["colpart_batch", [[], 4]]):
        assert R.plan_lines(lib, bad) is None, bad
    # ... and outside plan-only mode null pointers are an argument error
    for entry, d in (row, ["ln_bwd", [64, 640]], ["colsum", [64, 640, 1]], ["gn_sums_from_parts", [1, 300, 32]], ["colpart_batch", [[640], 4]]):
        lib.launch_log(1)
        try:
            assert R.call_row(lib, [entry, d]) == 1 and lib.launched() == []
        finally:
            lib.launch_log(0)
