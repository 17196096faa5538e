"""Host side of several policies in one fleet (sim2sim.FleetInfer with a list of policy files; DESIGN.md §9
"Policies"): the constructor's refusals, which are raised before any device work, the tiling of one segment's
tables, the per-policy report, the paired wins and the ranking on hand-made arrays, and the command line. No GPU."""

import json
import os

import numpy as np
import pytest
import torch

from open_duck_playground_amd import native, sim2sim
from open_duck_playground_amd.sim2sim import FleetInfer
from tests.fleet_policy_helpers import graph_file

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W = (101, 16, 14)     # obs -> hidden -> actions of the small hand-built policy files


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("policies")
    return {"a": graph_file(d / "a.onnx", W, 1), "b": graph_file(d / "b.onnx", W, 2),
            "wide": graph_file(d / "wide.onnx", (101, 24, 14), 3), "plain": graph_file(d / "plain.onnx", W, 4, normaliser=False),
            "deep": graph_file(d / "deep.onnx", (101, 8, 8, 8, 8, 14), 5)}


# --- the constructor's refusals ---------------------------------------------------------------
def test_header_declares_the_entry_and_the_limit():
    assert native.HEADERS.consts["DUCK_POLICY_MAX_POLICIES"] == 64
    assert "duck_policy_act_multi" in native.EXPORTS and "duck_policy_multi_order" in native.EXPORTS


def test_refusals_come_before_any_device_work(files):
    """Every refusal is raised while the files are read: no env exists yet, so none needs a GPU."""
    a, b = files["a"], files["b"]

    def refused(match, paths, n=6, **kw):
        with pytest.raises(native.DuckError, match=match):
            FleetInfer("flat_terrain", paths, n, device="cuda:0", **kw)
    refused("wide.onnx.*one architecture", [a, b, files["wide"]])
    refused("a.onnx.*normaliser.*plain.onnx.*none", [a, files["plain"]])
    refused("plain.onnx.*none", [files["plain"], a])
    refused("deep.onnx.*duck_policy_act's limits", [a, files["deep"]])
    refused("at most 64 policies", [a] * 65, n=65)
    refused("sum to 5, the fleet has 6", [a, b], policy_robots=(2, 3))
    refused("2 non-negative integers", [a, b], policy_robots=(2, 2, 2))
    refused("2 non-negative integers", [a, b], policy_robots=(7, -1))
    refused("do not split equally", [a, b], n=7)
    refused("at least one file", [])
    refused("a.onnx", [a, b], follow=(np.zeros((4, 115), np.float32), None))
    refused("equal segments", [a, b], randomize=0, policy_robots=(2, 4))
    refused("not a list", a, policy_robots=(6,))


def test_load_policies_and_segments(files):
    pols, seg = sim2sim.load_policies((files["a"], files["b"]), 10)
    assert len(pols) == 2 and pols[0]["sizes"] == [101, 16, 28] and seg.tolist() == [0, 5, 10] and seg.dtype == np.int32
    assert pols[0]["W"][0].tobytes() != pols[1]["W"][0].tobytes()
    assert sim2sim.policy_segments(3, 9, (0, 9, 0)).tolist() == [0, 0, 9, 9]
    assert sim2sim.policy_segments(1, 4).tolist() == [0, 4]


# --- tiling --------------------------------------------------------------------------------------
def test_tile_over_policies():
    a = np.arange(6, dtype=np.float32).reshape(3, 2)
    t = sim2sim.tile_over_policies(a, 4)
    assert t.shape == (12, 2) and t.dtype == np.float32
    for k in range(4):
        np.testing.assert_array_equal(t[3 * k:3 * k + 3], a)
    ids = sim2sim.tile_over_policies(np.array([2, 0, 1], np.int32), 2)
    assert ids.tolist() == [2, 0, 1, 2, 0, 1] and ids.dtype == np.int32
    np.testing.assert_array_equal(sim2sim.tile_over_policies(a, 1), a)


# --- the report ----------------------------------------------------------------------------------
def _acc(periods, lin=None):
    """acc [N][6]: periods survived, sums of vx, vy, wz, squared linear and yaw error."""
    periods = np.asarray(periods, np.float32)
    acc = np.zeros((len(periods), 6), np.float32)
    acc[:, 0] = periods
    acc[:, 4] = periods * (0.04 if lin is None else np.asarray(lin, np.float32))
    acc[:, 5] = periods * 0.25
    return acc


def _rep(periods, total):
    periods = np.asarray(periods, np.float64)
    return {"periods": periods, "fell": periods < total}


def test_policy_report_pools_over_the_segment():
    periods = [10, 10, 4, 10, 0, 0, 10, 6]
    acc, rep = _acc(periods, lin=[0.04, 0.16, 0.04, 0.04, 0, 0, 0.36, 0.36]), _rep(periods, 10)
    rows = sim2sim.policy_report(rep, acc, [0, 3, 4, 6, 6, 8], 10)
    assert [r["policy"] for r in rows] == [0, 1, 2, 3, 4] and [r["count"] for r in rows] == [3, 1, 2, 0, 2]
    assert rows[0]["survival_rate"] == pytest.approx(2 / 3) and rows[0]["mean_periods"] == pytest.approx(8.0)
    # pooled over the surviving periods, not a mean of per-robot rms values: (10 * .04 + 10 * .16 + 4 * .04) / 24
    assert rows[0]["rms_lin_err"] == pytest.approx(np.sqrt(2.16 / 24), rel=1e-6)
    assert rows[0]["rms_yaw_err"] == pytest.approx(0.5, rel=1e-6)
    assert rows[2]["survival_rate"] == 0.0 and rows[2]["mean_periods"] == 0.0 and rows[2]["rms_lin_err"] is None
    assert rows[3] == {"policy": 3, "count": 0, "survival_rate": None, "mean_periods": None, "periods": 10,
                       "rms_lin_err": None, "rms_yaw_err": None}
    assert rows[4]["rms_lin_err"] == pytest.approx(0.6, rel=1e-6)
    assert "cells" not in rows[0] and "pushes" not in rows[0] and "latency" not in rows[0]
    json.dumps(rows)


def test_policy_report_per_cell_rows_are_the_segments_own():
    """With tiled tables the per-cell rows of a segment are what grid_report, push_report and latency_report give
    for that segment's slice."""
    S, K, total = 6, 2, 10
    rng = np.random.default_rng(2)
    periods = rng.integers(0, total + 1, S * K)
    acc, rep = _acc(periods, lin=rng.uniform(0.01, 0.3, S * K)), _rep(periods, total)
    cells = sim2sim.command_grid("2x1x1")
    push_cell = sim2sim.tile_over_policies(np.arange(S) // 2 % 3, K)
    delay_cells = sim2sim.delay_grid("2x1")
    delay_cell = sim2sim.tile_over_policies(np.arange(S) % 2, K)
    rows = sim2sim.policy_report(rep, acc, [0, S, 2 * S], total, cells, (push_cell, 3, 0, 5), (delay_cell, delay_cells, False))
    for k, row in enumerate(rows):
        s = slice(S * k, S * (k + 1))
        sub = {key: v[s] for key, v in rep.items()}
        assert row["cells"] == sim2sim.grid_report(sub, acc[s], cells, total)
        assert row["pushes"] == sim2sim.push_report(sub, push_cell[s], 3, 0, total, 5)
        assert row["latency"] == sim2sim.latency_report(sub, acc[s], delay_cell[s], delay_cells, total, False)
        assert sum(c["count"] for c in row["cells"]) == S


def test_grid_report_with_cell_ids():
    periods = [10, 2, 10, 4, 10, 6]
    acc, rep = _acc(periods), _rep(periods, 10)
    cells = sim2sim.command_grid("2x1x1")
    assert sim2sim.grid_report(rep, acc, cells, 10, np.arange(6) % 2) == sim2sim.grid_report(rep, acc, cells, 10)
    rows = sim2sim.grid_report(rep, acc, cells, 10, [0, 0, 1, 0, 0, 1])
    assert [r["count"] for r in rows] == [4, 2] and rows[0]["mean_periods"] == pytest.approx(6.5)


def test_paired_wins_counts_strict_wins():
    #                 scenario 0  1  2  3
    periods = np.array([10, 5, 7, 0,      # policy 0
                        10, 6, 7, 0,      # policy 1
                        3, 9, 7, 0])      # policy 2
    w = sim2sim.paired_wins(periods, 3)
    assert w.dtype == np.int64
    assert w.tolist() == [[0, 0, 1], [1, 0, 1], [1, 1, 0]]          # ties count for neither
    assert sim2sim.paired_wins(periods, 1).tolist() == [[0]]
    assert sim2sim.paired_wins(np.array([1.0, np.nan, 2.0, 3.0]), 2).tolist() == [[0, 0], [1, 0]]   # NaN wins nothing
    with pytest.raises(native.DuckError, match="equal segments"):
        sim2sim.paired_wins(periods, 5)


def test_rank_policies_orders_by_survival_periods_error_index():
    row = lambda s, p, e: {"survival_rate": s, "mean_periods": p, "rms_lin_err": e}  # noqa: E731
    rows = [row(0.5, 8.0, 0.1),            # 0
            row(1.0, 10.0, 0.3),           # 1: the best survival, the larger error
            row(1.0, 10.0, 0.2),           # 2: ... the smaller error
            row(1.0, 10.0, None),          # 3: no error figure: after those with one
            row(1.0, 10.0, float("nan")),  # 4: NaN as None, the index decides
            row(0.5, 9.0, 0.9),            # 5: more periods than 0 at the same survival
            row(None, None, None),         # 6: no robots: last
            row(1.0, 10.0, 0.2)]           # 7: ties with 2: the index decides
    assert sim2sim.rank_policies(rows) == [2, 7, 1, 3, 4, 5, 0, 6]
    assert sim2sim.rank_policies([]) == []


def test_policies_doc_keys():
    periods = [10, 4, 10, 10]
    doc = sim2sim.policies_doc(["x.onnx", "y.onnx"], _rep(periods, 10), _acc(periods), [0, 2, 4], 10)
    assert sorted(doc) == ["paired_wins", "policies", "ranking"]
    assert [r["path"] for r in doc["policies"]] == ["x.onnx", "y.onnx"]
    assert doc["ranking"] == [1, 0] and doc["paired_wins"] == [[0, 0], [1, 0]]
    json.dumps(doc)


# --- the command line ----------------------------------------------------------------------------
@pytest.mark.parametrize("argv,message", [
    (["--policies", "a.onnx", "b.onnx", "-o", "c.onnx"], "takes the place of -o"),
    (["--policies", "a.onnx", "b.onnx", "--follow", "log.npz"], "cannot be combined with --follow"),
    (["--policies", "a.onnx", "b.onnx", "c.onnx", "--num_robots", "1024"], "not divisible by the 3 --policies"),
    (["--policies"] + ["a.onnx"] * 65 + ["--num_robots", "65"], "at most 64"),
    ([], "is required")])
def test_usage_errors(argv, message, capsys):
    with pytest.raises(SystemExit) as e:
        sim2sim.parse_arguments(argv)
    assert e.value.code == 2 and message in capsys.readouterr().err


def test_policies_flag_parses():
    args = sim2sim.parse_arguments(["--policies", "a.onnx", "b.onnx", "--num_robots", "6"])
    assert args.policies == ["a.onnx", "b.onnx"] and args.onnx_model_path is None and args.num_robots == 6
    assert sim2sim.parse_arguments(["-o", "a.onnx"]).policies is None


class _Fleet:
    """What main() asks of a fleet, on the host: it keeps what it was given and reports a fixed outcome."""
    made = []

    def __init__(self, model_path, onnx_model_path, num_robots, **kw):
        self.paths, self.n, self.kw, self.set = onnx_model_path, num_robots, kw, {}
        K = len(onnx_model_path) if isinstance(onnx_model_path, list) else 1
        self.num_policies, self.policy_seg = K, sim2sim.policy_segments(K, num_robots)
        self.dr, self.num_dofs = None, 14
        periods = (np.arange(num_robots) * 7) % 11
        self.acc = torch.tensor(_acc(periods))
        self._rep = _rep(periods, 10)
        _Fleet.made.append(self)

    def run(self, periods):
        self.periods = periods

    def report(self):
        return self._rep

    def __getattr__(self, name):
        if not name.startswith("set_"):
            raise AttributeError(name)
        return lambda *a: self.set.__setitem__(name, a)


def test_report_keys_only_with_the_flag(monkeypatch, tmp_path, capsys):
    """main() with a host stand-in for the fleet: without --policies the report has none of the three keys and the
    tables are built for all robots; with it they are there, every table is one segment's, tiled, and --num_robots
    stays the total."""
    monkeypatch.setattr(sim2sim, "FleetInfer", _Fleet)
    _Fleet.made.clear()
    out = str(tmp_path / "report.json")
    common = ["--periods", "10", "--command_grid", "2x2x1", "--push_grid", "1x2", "--push_at", "3", "--delay_grid", "2x1",
              "--out", out]
    assert sim2sim.main(["-o", "a.onnx", "--num_robots", "12"] + common) == 0
    doc = json.load(open(out))
    assert not {"policies", "ranking", "paired_wins"} & set(doc) and doc["onnx_model_path"] == "a.onnx"
    plain = _Fleet.made[-1]
    assert plain.paths == "a.onnx" and plain.set["set_commands"][0].shape == (12, 7)

    assert sim2sim.main(["--policies", "a.onnx", "b.onnx", "c.onnx", "--num_robots", "36"] + common) == 0
    capsys.readouterr()
    doc = json.load(open(out))
    fleet = _Fleet.made[-1]
    assert fleet.paths == ["a.onnx", "b.onnx", "c.onnx"] and fleet.n == 36 and doc["num_robots"] == 36
    assert [r["path"] for r in doc["policies"]] == ["a.onnx", "b.onnx", "c.onnx"] and [r["count"] for r in doc["policies"]] == [12] * 3
    assert sorted(doc["ranking"]) == [0, 1, 2] and np.array(doc["paired_wins"]).shape == (3, 3)
    assert all(k in doc["policies"][0] for k in ("cells", "pushes", "latency", "survival_rate", "mean_periods", "rms_lin_err"))
    # one segment's tables, three times: those of the 12-robot fleet above
    cmd, = fleet.set["set_commands"]
    assert cmd.shape == (36, 7)
    for k in range(3):
        np.testing.assert_array_equal(cmd[12 * k:12 * k + 12], plain.set["set_commands"][0])
        for mine, theirs in zip(fleet.set["set_pushes"], plain.set["set_pushes"]):
            np.testing.assert_array_equal(np.broadcast_to(mine, (36,))[12 * k:12 * k + 12], np.broadcast_to(theirs, (12,)))
        for mine, theirs in zip(fleet.set["set_latency"][:2], plain.set["set_latency"][:2]):
            np.testing.assert_array_equal(mine[12 * k:12 * k + 12], theirs)
    # the fleet-wide rows count every robot once, in its own cell
    assert sum(c["count"] for c in doc["cells"]) == 36 and [c["count"] for c in doc["cells"]] == [9] * 4
    assert sum(c["count"] for c in doc["pushes"]) == 36 and sum(c["count"] for c in doc["latency"]) == 36
