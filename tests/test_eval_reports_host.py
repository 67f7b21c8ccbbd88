"""utils/eval_reports.py and options.EVAL_TABLE on the host: for every report and every combination of the switches that append a
column group, the record of a batch is as wide as the empty block a rank without a sample joins the gather with, the category sits in
the declared column and the declared files are the ones written; every row of the settings table accepts its default and refuses what
is outside its kind, whether or not the switch it belongs to is on."""
import itertools
import os
import types

import pytest
import torch

from shapeclipper_amd.utils import eval_reports, options
from shapeclipper_amd.utils.util import EasyDict as edict

B = 3
IDX, CATEGORY = [4, 7, 9], [1, 0, 1]


def _values(keys, first, suffix=""):
    return {k + suffix: torch.arange(B, dtype=torch.float32) + first + i for i, k in enumerate(keys)}


def _stats(first):
    return {k: torch.arange(B, dtype=torch.float64) + first + i for i, k in enumerate(eval_reports.MESH_STATS_KEYS)}


def _var(icp, dual, stats, n_th):
    """What eval_metrics and dump_geometry leave in var with every output on, under the three switches that append a column group."""
    var = edict(idx=torch.tensor(IDX), category_label=torch.tensor(CATEGORY))
    var.component_stats = _values(eval_reports.COMPONENT_KEYS, 100)
    var.update(_values(("cd_acc", "cd_comp", "cd_comp_mesh", "nc_acc", "nc_comp", "nc", "emd", "emd_rounds", "emd_converged"), 200))
    var.update(_values(eval_reports.IOU_KEYS, 300), emd_n=64, iou_res=32, f_score_mesh=torch.rand(B, n_th))
    var.mesh_simplified = dict(_values(eval_reports.SIMPLIFY_KEYS, 400), cell=2)
    var.texture = [types.SimpleNamespace(stats=dict(faces=10 + b, atlas=64, rows=3, err_mean=0.25, err_max=0.5)) for b in range(B)]
    var.mesh_render = types.SimpleNamespace(faces=[10, 11, 12], pixels=[5, 0, 7], iou_input=torch.tensor([0.5, float("nan"), 1.0]),
                                            iou_volume=torch.rand(B))
    if icp:
        var.icp = dict(transform=torch.eye(4).repeat(B, 1, 1), s=torch.ones(B), objective=torch.rand(B, 5))
        var.update(_values(("cd_acc", "cd_comp", "nc_acc", "nc_comp", "nc", "emd", "emd_rounds", "emd_converged"), 500, "_icp"))
        var.update(_values(eval_reports.IOU_KEYS, 600, "_icp"), f_score_icp=torch.rand(B, n_th))
    if dual:
        var.update(cd_comp_dual=torch.rand(B), f_score_dual=torch.rand(B, n_th))
    if stats:
        var.mesh_stats, var.mesh_stats_simplified = _stats(700), _stats(800)
        if dual:
            var.mesh_stats_dual = _stats(900)
    return var


def _opt(icp, dual, stats, n_th, path):
    return edict(output_path=str(path), data=dict(num_classes=2), hip=dict(largest_component=True),
                 eval=dict(icp=icp, dual_mesh=dual, mesh_stats=stats, f_thresholds=[0.01 * (i + 1) for i in range(n_th)], normals=True,
                           mesh_dist=True, emd=True, iou=True, simplify=2, texture=True, mesh_render=True))


@pytest.mark.parametrize("report", eval_reports.REPORTS, ids=lambda rep: rep.key)
@pytest.mark.parametrize("icp,dual,stats,n_th", list(itertools.product((False, True), (False, True), (False, True), (6, 2))))
def test_width_equals_records(report, icp, dual, stats, n_th, tmp_path, monkeypatch):
    monkeypatch.setattr(eval_reports, "util_vis", object())             # texture and mesh_render gather only where the dumps can be written
    opt, var = _opt(icp, dual, stats, n_th, tmp_path), _var(icp, dual, stats, n_th)
    on = {"icp": icp, "mesh_stats": stats}.get(report.key, True)
    assert bool(report.enabled(opt)) == report.present(var, opt) == on
    if not on:
        return
    rec = report.records(var)
    assert rec.dtype == torch.float64 and rec.shape == (B, report.width(opt))
    assert torch.cat([torch.zeros(0, report.width(opt), dtype=torch.float64), rec]).shape == rec.shape      # a rank without a sample
    at = report.layout(opt)
    assert rec[:, at["idx"]].tolist() == IDX and at["idx"] == 0
    if eval_reports.CAT in at:
        assert rec[:, at[eval_reports.CAT]].tolist() == CATEGORY
    else:
        assert not any(g.tables for g in report.groups(opt))
    groups = report.groups(opt)
    assert len(groups) == 1 + (report.extra is not None and {"_icp": icp, "dual": dual, "simplified": stats}[
        [k for k in ("_icp", "dual", "simplified") if k in report.extra.marker][0]])
    report.write_lines(opt.output_path, rec, "w", opt)
    report.write_lines(opt.output_path, rec, "a", opt)
    files = sorted(f.name for g in groups for f in g.files)
    assert sorted(os.listdir(tmp_path)) == files
    for g in groups:
        for f in g.files:
            lines = open(tmp_path / f.name).read().splitlines()
            assert [l.split()[0] for l in lines] == [str(i) for i in IDX] * 2 and all(len(l.split()) == f.line.count("%") for l in lines)
    report.write(opt, rec, {0: "chair", 1: "sofa"}, per_sample=False)
    tables = [t.name for g in groups for t in g.tables] + [g.f_score[0] for g in groups if g.f_score]
    assert sorted(os.listdir(tmp_path)) == sorted(files + tables)
    for g in groups:
        for t in g.tables:
            lines = open(tmp_path / t.name).read().splitlines()
            assert lines[0] + "\n" == t.header and [l.split()[-2:] for l in lines[1:]] == [["1", "chair"], ["2", "sofa"]]
    with pytest.raises(ValueError, match=report.key):                   # a row of another width belongs to no combination
        report.write_lines(opt.output_path, rec[:, :-1], "w", opt)


def test_reports_are_in_the_order_of_the_gathers():
    assert [rep.key for rep in eval_reports.REPORTS] == ["components", "icp", "normals", "mesh_dist", "emd", "iou", "mesh_stats", "simplify",
                                                         "texture", "mesh_render"]
    assert [rep.marker for rep in eval_reports.REPORTS] == ["component_stats", "icp", "nc", "cd_comp_mesh", "emd", "iou", "mesh_stats",
                                                            "mesh_simplified", "texture", "mesh_render"]
    off = edict(eval=dict(f_thresholds=[0.1]))
    assert not any(rep.enabled(off) for rep in eval_reports.REPORTS)
    var = _var(False, False, False, 1)                                  # --eval.mesh_render alone bakes var.texture and writes no texture.txt
    assert not eval_reports.REPORT["texture"].present(var, off) and eval_reports.REPORT["mesh_render"].present(var, off)


# ---- the settings table ------------------------------------------------------------------------------------------------------------------
# key -> (the function that answers for it, what turns its switch on, what turns it off)
OWNER = {"texture_texels": ("texture_texels", dict(texture=True), {}), "dual_reg": ("dual_mesh_reg", dict(dual_mesh=True), {}),
         "icp_iters": ("icp_settings", dict(icp=True), {}), "normals_k": ("normal_settings", dict(normals=True), {}),
         "emd_points": ("emd_settings", dict(emd=True), {}), "emd_eps": ("emd_settings", dict(emd=True), {}),
         "iou_res": ("iou_settings", dict(iou=True), {}), "iou_close": ("iou_settings", dict(iou=True), {}),
         "simplify": ("simplify_settings", {}, {}), "simplify_reg": ("simplify_settings", dict(simplify=2), {})}


def test_the_table_has_a_row_per_setting():
    assert [row.key for row in options.EVAL_TABLE] == [
        "texture", "texture_texels", "mesh_render", "dual_mesh", "dual_reg", "icp", "icp_iters", "icp_scale", "normals", "normals_k", "mesh_dist",
        "emd", "emd_points", "emd_eps", "iou", "iou_res", "iou_close", "mesh_stats", "simplify", "simplify_reg"]
    assert sorted(k for k, row in options.EVAL.items() if row.kind is not bool) == sorted(OWNER)
    assert {row.key: row.flag for row in options.EVAL_TABLE if row.flag} == {"emd_eps": "str", "simplify_reg": "str", "simplify": "absent"}


@pytest.mark.parametrize("row", options.EVAL_TABLE, ids=lambda row: row.key)
def test_every_row_accepts_its_default_and_refuses_what_is_outside_its_kind(row):
    name = "eval.%s must be " % row.key
    for tree in (edict(), edict(eval={}), edict(eval={row.key: row.default})):
        assert options.eval_setting(tree, row.key) == row.default
    if row.kind is bool:
        assert options.eval_setting(edict(eval={row.key: not row.default}), row.key) is (not row.default)
        for bad in (1, 0, "yes", None, 1.0):
            with pytest.raises(ValueError, match=name + "a bool"):
                options.eval_setting(edict(eval={row.key: bad}), row.key)
        return
    lo, hi = row.kind
    if isinstance(lo, int):
        good, bad, what = (lo, hi), (True, lo + 0.5, float(lo), lo - 1, hi + 1, str(lo), None), "an integer in %d..%d" % (lo, hi)
        if row.flag == "absent":
            bad = bad[:-1]
    else:
        good, bad, what = (hi, hi / 2, 1e-9), (True, lo, lo - 1, hi + 1, "small", None, float("nan")), "a float in (%g, %g]" % (lo, hi)
        assert type(options.eval_setting(edict(eval={row.key: hi}), row.key)) is float
        if row.flag == "str":
            assert options.eval_setting(edict(eval={row.key: "1e-4"}), row.key) == 1e-4
        else:
            bad += ("1e-4",)
    function, on, off = OWNER[row.key]
    for value in good:
        assert options.eval_setting(edict(eval={row.key: value}), row.key) == value
    for value in bad:
        for switch in (on, off):                                        # refused whether or not the switch is on
            with pytest.raises(ValueError) as e:
                getattr(options, function)(edict(eval=dict(switch, **{row.key: value})))
            assert str(e.value).startswith(name + what + ", got ")


@pytest.mark.parametrize("key,value,message", [("iou_res", 7, "eval.iou_res must be an integer in 8..64, got 7"),
                                               ("dual_reg", 1.5, "eval.dual_reg must be a float in (0, 1], got 1.5"),
                                               ("texture", "yes", "eval.texture must be a bool, got 'yes'"),
                                               ("emd_eps", "0.5", "eval.emd_eps must be a float in (0, 0.25], got 0.5"),
                                               ("simplify", True, "eval.simplify must be an integer in 2..16, got True")])
def test_the_messages_are_the_ones_raised_before_the_table(key, value, message):
    with pytest.raises(ValueError) as e:
        options.eval_setting(edict(eval={key: value}), key)
    assert str(e.value) == message
