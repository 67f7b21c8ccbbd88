"""The optional outputs of an evaluation, one row of REPORTS each: which key of `var` marks that a batch carries it, whether every rank must
join its gather, the columns of its per-sample record, and the files written from those records.  Host code only: records are float64
tensors on the host (the counts are exact in it), and nothing here launches a kernel.

A record is the report's base columns followed, when another switch adds them, by ONE further group of columns (the values after ICP,
those of the dual-contouring mesh, the statistics of the simplified mesh).  records(var), width(opt), every column index a writer uses
and the files a row of a given width yields are all computed from the same declaration, so the empty [0, width] block with which a
rank without a sample joins a gather cannot drift from what records() stacks.  Runner.dump_results appends the per-sample lines of a
batch (write_lines), Runner.evaluate writes the per-category tables (write(per_sample=False)) and Runner.evaluate_sharded both, from
the gathered rows (write)."""
from __future__ import annotations

import collections
import functools
import os
import re

import torch

from . import options

try:
    from . import util_vis
except Exception:  # pragma: no cover
    util_vis = None

T = "T"                                       # the width of a column that holds a value per entry of eval.f_thresholds

CHAMFER_LINE = "%d %.8f %.8f\n"              # a line of chamfer_icp.txt: idx cd_acc cd_comp
ICP_LINE = "%d %.8f %.8f %.8f %.8f %.8f\n"   # a line of icp.txt: idx s angle_deg |t| objective first, last
COMPONENTS_LINE = "%d %d %d %d\n"            # a line of components.txt: idx n_components inside_voxels kept_voxels
NC_LINE = "%d %.8f %.8f %.8f\n"              # a line of normal_consistency.txt: idx nc_acc nc_comp nc
MESH_LINE = "%d %.8f %.8f\n"                  # a line of completeness_mesh.txt: idx cd_comp cd_comp_mesh
EMD_LINE = "%d %d %.8f %d %d\n"              # a line of emd.txt: idx n emd rounds converged
IOU_LINE = "%d %d %.8f %d %d %d %d %d %d\n"  # a line of iou.txt: idx res iou inter union vox_pred vox_gt shell_pred shell_gt
# a line of mesh_stats.txt: idx vertices faces edges boundary nonmanifold_edges nonmanifold_vertices inconsistent degenerate unreferenced
# components largest_faces euler genus watertight oriented manifold area volume
MESH_STATS_LINE = "%d" + " %d" * 16 + " %.8f %.8f\n"
# a line of simplify.txt: idx cell vertices_in vertices_out faces_in faces_out collapsed cancelled dist_mean dist_max
SIMPLIFY_LINE = "%d" + " %d" * 7 + " %.8f %.8f\n"
TEXTURE_LINE = "%d %d %d %d %.6f %.6f\n"     # a line of texture.txt: idx faces atlas rows err_mean err_max
MESH_RENDER_LINE = "%d %d %d %.6f %.6f\n"   # a line of mesh_render.txt: idx faces pixels iou_input iou_volume

COMPONENT_KEYS = ("n_components", "inside_voxels", "kept_voxels")
ICP_KEYS = ("icp_s", "icp_angle", "icp_shift", "icp_first", "icp_last")
IOU_KEYS = ("iou", "iou_inter", "iou_union", "iou_vox_pred", "iou_vox_gt", "iou_shell_pred", "iou_shell_gt")
MESH_STATS_KEYS = ("vertices", "faces", "edges", "boundary_edges", "nonmanifold_edges", "nonmanifold_vertices", "inconsistent_edges",
                   "degenerate_faces", "unreferenced_vertices", "components", "largest_component_faces", "euler", "genus", "watertight",
                   "oriented", "manifold", "area", "volume")
SIMPLIFY_KEYS = ("vertices_in", "v_count", "faces_in", "f_count", "collapsed", "cancelled", "dist_mean", "dist_max")
TEXTURE_KEYS = ("faces", "atlas", "rows", "err_mean", "err_max")


def icp_summary(var):
    """[B,5] float64 on the host, a row of icp.txt per sample: s, the rotation angle in degrees, |t|, the first and the last objective."""
    M, s, obj = (var.icp[k].detach().cpu().double() for k in ("transform", "s", "objective"))
    cos = ((M[:, 0, 0] + M[:, 1, 1] + M[:, 2, 2]) / s - 1) / 2
    angle = torch.rad2deg(torch.acos(cos.clamp(-1, 1)))
    return torch.stack([s, angle, M[:, :3, 3].norm(dim=1), obj[:, 0], obj[:, -1]], dim=1)


def _component_counts(var):
    """(n_components, inside_voxels, kept_voxels) [B] of var.component_stats (eval_3D.eval_metrics with `--hip.largest_component`)."""
    return tuple(var.component_stats[k] for k in COMPONENT_KEYS)


def _fetch(src, name):
    """src.a.b of the column "a.b" (items of a dict, attributes of anything else); a list on the way gives the list of its elements' values."""
    parts = name.split(".")
    for i, part in enumerate(parts):
        if isinstance(src, list):
            return [_fetch(x, ".".join(parts[i:])) for x in src]
        src = src[part] if isinstance(src, dict) else getattr(src, part)
    return src


def _stack(src, cols, B):
    """[B, width of cols] float64 on the host: the columns `cols` of src side by side; a plain number stands for every sample."""
    out = []
    for name, w in cols:
        v = _fetch(src, name)
        if not isinstance(v, torch.Tensor):
            v = torch.tensor([float(x) for x in v] if isinstance(v, list) else float(v), dtype=torch.float64)
        v = v.detach().double().cpu()
        out.append(v.expand(B, 1) if v.dim() == 0 else v.reshape(B, -1 if w is T else w))
    return torch.cat(out, dim=1)


@functools.lru_cache(maxsize=None)
def _kinds(line):
    return re.findall(r"%[.\d]*([df])", line)


def _line(line, r, cols):
    """`line` filled from the columns `cols` of the row r: int() where it says %d, float() where it says %f."""
    return line % tuple(int(r[c]) if k == "d" else float(r[c]) for k, c in zip(_kinds(line), cols))


def _means(sel, n, cols):
    """Per-category values in cd_cat.txt's style: the mean of every column (count + 0.001 in the denominator), two columns preceded by
    the mean of the two."""
    v = [float(sel[:, c].sum()) / n for c in cols]
    return ([(v[0] + v[1]) / 2] if len(v) == 2 else []) + v


def _closed_comps_genus(sel, n, cols):
    """mesh_stats_cat.txt: the share of samples whose mesh is watertight and manifold, the mean number of components, and the mean genus
    over the samples whose genus is >= 0 (0 when there is none)."""
    comps, genus, water, manifold = cols
    g = sel[sel[:, genus] >= 0][:, genus]
    return [float(((sel[:, water] != 0) & (sel[:, manifold] != 0)).sum()) / n, float(sel[:, comps].sum()) / n,
            float(g.sum()) / (g.shape[0] + 0.001)]


File = collections.namedtuple("File", ["name", "line", "fields"])                     # a per-sample file: a `line` of `fields` per row
# a per-category table: header, then a line per category of rule(rows of the category, count + 0.001, columns of `fields`) as %.4f, the
# count as %5d and the category's name
Table = collections.namedtuple("Table", ["name", "header", "fields", "rule"], defaults=(_means,))
# columns ("name" or ("name", width)) with the files written from them; the group a switch appends also says which key of var marks it
# (`marker`), which setting turns it on (`on(opt)`), and may name an F-score file (name, its T-wide column)
Group = collections.namedtuple("Group", ["cols", "files", "tables", "f_score", "marker", "on"], defaults=((), None, None, None))
CAT = "category_label"
CD_HEADER = "CD     Acc    Comp   Count Cat\n"


class Report:
    """A row of REPORTS.  key names it; `marker` in var says a batch carries it (`present` adds a condition on opt); enabled(opt) says
    that every rank joins its gather; base and extra are its Groups; source(var), where given, is what the columns are fetched from."""

    def __init__(self, key, marker, enabled, base, extra=None, source=None, present=None):
        self.key, self.marker, self.enabled, self.source, self._also = key, marker, enabled, source, present
        norm = lambda g: g._replace(cols=tuple(c if isinstance(c, tuple) else (c, 1) for c in g.cols))
        self.base, self.extra = norm(base), None if extra is None else norm(extra)

    def present(self, var, opt):
        return self.marker in var and (self._also is None or self._also(opt))

    def groups(self, opt):
        """The groups of a record under these settings."""
        return (self.base,) + ((self.extra,) if self.extra is not None and self.extra.on(opt) else ())

    def _width(self, group, opt):
        return sum(len(opt.eval.f_thresholds) if w is T else w for _, w in group.cols)

    def width(self, opt):
        return sum(self._width(g, opt) for g in self.groups(opt))

    def layout(self, opt=None):
        """{column: its first index} in a row that carries every group (opt is read only where a column is T wide)."""
        at, n = {}, 0
        for g in (self.base,) + ((self.extra,) if self.extra is not None else ()):
            for name, w in g.cols:
                at[name], n = n, n + (len(opt.eval.f_thresholds) if w is T else w)
        return at

    def _groups_of(self, rows, opt):
        """The groups that rows of this width carry."""
        base = self._width(self.base, opt)
        if rows.shape[1] == base:
            return (self.base,)
        if self.extra is None or rows.shape[1] != base + self._width(self.extra, opt):
            raise ValueError("%s: records of %d columns" % (self.key, rows.shape[1]))
        return (self.base, self.extra)

    def records(self, var, extra=True):
        """[B, width] float64 on the host, a record per sample; extra=False leaves the appended group out."""
        groups = (self.base,) + ((self.extra,) if extra and self.extra is not None and self.extra.marker in var else ())
        return _stack(var if self.source is None else self.source(var), [c for g in groups for c in g.cols], len(var.idx))

    def write_lines(self, path, rows, mode="w", opt=None):
        """The per-sample files under `path` from rows in sample order."""
        at = self.layout(opt)
        for g in self._groups_of(rows, opt):
            for name, line, fields in g.files:
                cols = [at[k] for k in fields]
                with open(os.path.join(path, name), mode) as f:
                    for r in rows:
                        f.write(_line(line, r, cols))

    def write(self, opt, rows, names, per_sample=True):
        """Every file of the report under opt.output_path from rows in sample order: the per-sample files (per_sample=False leaves them to
        dump_results), the per-category tables with names[c] as the categories' names, and the F-score file."""
        if per_sample:
            self.write_lines(opt.output_path, rows, "w", opt)
        at = self.layout(opt)
        for g in self._groups_of(rows, opt):
            for name, header, fields, rule in g.tables:
                cols = [at[k] for k in fields]
                with open(os.path.join(opt.output_path, name), "w") as f:
                    f.write(header)
                    for c in range(opt.data.num_classes):
                        sel = rows[rows[:, at[CAT]] == c]
                        n = sel.shape[0] + 0.001
                        v = rule(sel, n, cols)
                        f.write("%.4f " * len(v) % tuple(v) + "%5d %s\n" % (n, names[c]))
            if g.f_score is not None:               # f_score.txt's format: precision from the samples, recall from the mesh
                name, first = g.f_score[0], at[g.f_score[1]]
                n_th = len(opt.eval.f_thresholds)
                fs = rows[:, first:first + n_th].mean(dim=0) if rows.shape[0] else torch.zeros(n_th, dtype=torch.float64)
                with open(os.path.join(opt.output_path, name), "w") as f:
                    for i, th in enumerate(opt.eval.f_thresholds):
                        f.write("F-score @ %.2f: %.4f\n" % (th * 100, fs[i].item()))


def _icp_on(opt):
    return options.icp_settings(opt) is not None


def _dual_on(opt):
    return options.dual_mesh_reg(opt) is not None


def _with(keys, suffix):
    return tuple(k + suffix for k in keys)


def _stats(key):
    return tuple("%s.%s" % (key, k) for k in MESH_STATS_KEYS)


def _stats_cat(key):
    return tuple("%s.%s" % (key, k) for k in ("components", "genus", "watertight", "manifold"))


_COMPONENTS = ("idx",) + tuple("component_stats." + k for k in COMPONENT_KEYS)
_NC, _EMD = ("nc_acc", "nc_comp", "nc"), ("emd", "emd_rounds", "emd_converged")
_SIMPLIFY = ("idx", "mesh_simplified.cell") + tuple("mesh_simplified." + k for k in SIMPLIFY_KEYS)
_TEXTURE = ("idx",) + tuple("texture.stats." + k for k in TEXTURE_KEYS)
_MESH_RENDER = ("idx",) + tuple("mesh_render." + k for k in ("faces", "pixels", "iou_input", "iou_volume"))
STATS_HEADER = "Closed Comps   Genus  Count Cat\n"

# In the order of the collectives of Runner.evaluate_sharded, which every rank must share.
REPORTS = (
    # --hip.largest_component
    Report("components", "component_stats", lambda opt: bool(options.hip(opt, "largest_component")),
           Group(_COMPONENTS, (File("components.txt", COMPONENTS_LINE, _COMPONENTS),))),
    # --eval.icp: the aligned metrics (evaluate() tallies cd_cat_icp.txt / f_score_icp.txt itself, evaluate_sharded through
    # Runner._write_gathered from the columns in front of ICP_KEYS), then icp.txt's five numbers
    Report("icp", "icp", _icp_on,
           Group(("idx", "cd_acc_icp", "cd_comp_icp", ("f_score_icp", T), CAT) + ICP_KEYS,
                 (File("chamfer_icp.txt", CHAMFER_LINE, ("idx", "cd_acc_icp", "cd_comp_icp")), File("icp.txt", ICP_LINE, ("idx",) + ICP_KEYS))),
           source=lambda var: dict(var, **dict(zip(ICP_KEYS, icp_summary(var).unbind(1))))),
    # --eval.normals: nc_cat.txt is cd_cat.txt's format
    Report("normals", "nc", lambda opt: options.normal_settings(opt) is not None,
           Group(("idx",) + _NC + (CAT,), (File("normal_consistency.txt", NC_LINE, ("idx",) + _NC),),
                 (Table("nc_cat.txt", "NC     Acc    Comp   Count Cat\n", _NC[:2]),)),
           Group(_with(_NC, "_icp"), (File("normal_consistency_icp.txt", NC_LINE, ("idx",) + _with(_NC, "_icp")),),
                 (Table("nc_cat_icp.txt", "NC     Acc    Comp   Count Cat\n", _with(_NC[:2], "_icp")),), marker="nc_icp", on=_icp_on)),
    # --eval.mesh_dist: cd_cat_mesh.txt is cd_cat.txt with Comp replaced by the mesh value
    Report("mesh_dist", "cd_comp_mesh", lambda opt: options.mesh_dist_settings(opt) is not None,
           Group(("idx", "cd_acc", "cd_comp", "cd_comp_mesh", ("f_score_mesh", T), CAT),
                 (File("completeness_mesh.txt", MESH_LINE, ("idx", "cd_comp", "cd_comp_mesh")),),
                 (Table("cd_cat_mesh.txt", CD_HEADER, ("cd_acc", "cd_comp_mesh")),), ("f_score_mesh.txt", "f_score_mesh")),
           Group(("cd_comp_dual", ("f_score_dual", T)), (File("completeness_mesh_dual.txt", MESH_LINE, ("idx", "cd_comp", "cd_comp_dual")),),
                 (Table("cd_cat_mesh_dual.txt", CD_HEADER, ("cd_acc", "cd_comp_dual")),), ("f_score_mesh_dual.txt", "f_score_dual"),
                 marker="cd_comp_dual", on=_dual_on)),
    # --eval.emd
    Report("emd", "emd", lambda opt: options.emd_settings(opt) is not None,
           Group(("idx", "emd_n") + _EMD + (CAT,), (File("emd.txt", EMD_LINE, ("idx", "emd_n") + _EMD),),
                 (Table("emd_cat.txt", "EMD    Count Cat\n", _EMD[:1]),)),
           Group(_with(_EMD, "_icp"), (File("emd_icp.txt", EMD_LINE, ("idx", "emd_n") + _with(_EMD, "_icp")),),
                 (Table("emd_cat_icp.txt", "EMD    Count Cat\n", _with(_EMD[:1], "_icp")),), marker="emd_icp", on=_icp_on)),
    # --eval.iou
    Report("iou", "iou", lambda opt: options.iou_settings(opt) is not None,
           Group(("idx", "iou_res") + IOU_KEYS + (CAT,), (File("iou.txt", IOU_LINE, ("idx", "iou_res") + IOU_KEYS),),
                 (Table("iou_cat.txt", "IoU    Count Cat\n", IOU_KEYS[:1]),)),
           Group(_with(IOU_KEYS, "_icp"), (File("iou_icp.txt", IOU_LINE, ("idx", "iou_res") + _with(IOU_KEYS, "_icp")),),
                 (Table("iou_cat_icp.txt", "IoU    Count Cat\n", _with(IOU_KEYS[:1], "_icp")),), marker="iou_icp", on=_icp_on)),
    # --eval.mesh_stats: the marching-cubes mesh, with --eval.dual_mesh the dual-contouring mesh behind it
    Report("mesh_stats", "mesh_stats", options.mesh_stats_settings,
           Group(("idx",) + _stats("mesh_stats") + (CAT,), (File("mesh_stats.txt", MESH_STATS_LINE, ("idx",) + _stats("mesh_stats")),),
                 (Table("mesh_stats_cat.txt", STATS_HEADER, _stats_cat("mesh_stats"), _closed_comps_genus),)),
           Group(_stats("mesh_stats_dual"), (File("mesh_stats_dual.txt", MESH_STATS_LINE, ("idx",) + _stats("mesh_stats_dual")),),
                 (Table("mesh_stats_cat_dual.txt", STATS_HEADER, _stats_cat("mesh_stats_dual"), _closed_comps_genus),),
                 marker="mesh_stats_dual", on=_dual_on)),
    # --eval.simplify: with --eval.mesh_stats the simplified mesh's statistics behind it, in mesh_stats.txt's format
    Report("simplify", "mesh_simplified", lambda opt: options.simplify_settings(opt) is not None,
           Group(_SIMPLIFY + (CAT,), (File("simplify.txt", SIMPLIFY_LINE, _SIMPLIFY),)),
           Group(_stats("mesh_stats_simplified"),
                 (File("mesh_stats_simplified.txt", MESH_STATS_LINE, ("idx",) + _stats("mesh_stats_simplified")),),
                 marker="mesh_stats_simplified", on=options.mesh_stats_settings)),
    # --eval.texture: var.texture is left by dump_geometry (--eval.mesh_render alone bakes it too and writes no texture.txt)
    Report("texture", "texture", lambda opt: options.texture_texels(opt) is not None and util_vis is not None,
           Group(_TEXTURE, (File("texture.txt", TEXTURE_LINE, _TEXTURE),)), present=lambda opt: options.texture_texels(opt) is not None),
    # --eval.mesh_render: var.mesh_render is left by dump_geometry; the IoUs are nan where the map to compare with is missing
    Report("mesh_render", "mesh_render", lambda opt: options.mesh_render(opt) and util_vis is not None,
           Group(_MESH_RENDER, (File("mesh_render.txt", MESH_RENDER_LINE, _MESH_RENDER),))),
)
REPORT = {rep.key: rep for rep in REPORTS}

# ---- the names the per-output tests and tools use ----------------------------------------------------------------------------------------
_normal_records = REPORT["normals"].records
_mesh_records = REPORT["mesh_dist"].records
_iou_records = REPORT["iou"].records
_mesh_stats_rows = REPORT["mesh_stats"].records
_write_mesh_stats_lines = REPORT["mesh_stats"].write_lines
# the columns of a line of iou.txt / iou_icp.txt behind idx and res
IOU_COLS = tuple((suffix, [REPORT["iou"].layout()[k + suffix] for k in IOU_KEYS]) for suffix in ("", "_icp"))


def _mesh_stats_records(var, key="mesh_stats"):
    """[B,20] float64 on the host, a record per sample of eval_3D.mesh_stats' result var[key]: idx, the 18 values of MESH_STATS_KEYS, category."""
    return _stack(var, [(c, 1) for c in ("idx",) + _stats(key) + (CAT,)], len(var.idx))


def iou_line(r, cols):
    """The line of iou.txt (or iou_icp.txt) of one row of _iou_records."""
    return _line(IOU_LINE, r, [0, 1] + list(cols))


def mesh_stats_line(r, first=1):
    """The line of mesh_stats.txt (or mesh_stats_dual.txt: first = the dual mesh's first column) of one row of _mesh_stats_rows."""
    return _line(MESH_STATS_LINE, r, [0] + list(range(first, first + len(MESH_STATS_KEYS))))
