"""Training / evaluation engine -- call surface of the reference's model/runner.py
(Runner: load_dataset, build_networks, setup_optimizer, restore_checkpoint, setup_visualizer,
train, evaluate, ...).  Differences that matter on MI355X:

  * data parallelism is one process per GPU with ONE flat RCCL all-reduce of all gradients per step
    (shapeclipper_amd/parallel.py) instead of DistributedDataParallel's bucketed reducer;
  * the per-loss `.mean()` + isnan/isinf asserts (two host syncs per loss key, runner.py:294-305) are
    folded into a single device-side check that is read once per step;
  * TensorBoard / image dumps are optional (used when importable), never required by the step.
"""
from __future__ import annotations

import contextlib
import functools
import importlib
import os
import shutil
import time
from copy import deepcopy

import numpy as np
import torch
import tqdm

from ..data.pix3d import sample_rays_device
from ..parallel import FlatGradAllReduce, ModuleHolder
from ..utils import eval_3D, options, util
from ..utils.util import EasyDict as edict
from ..utils.util import cleanup, log, setup
# the optional evaluation outputs are declared in utils/eval_reports.py; the names the per-output tests and tools import stay reachable here
from ..utils.eval_reports import (ICP_KEYS, IOU_COLS, IOU_KEYS, MESH_LINE, MESH_STATS_KEYS, MESH_STATS_LINE, NC_LINE, REPORT, REPORTS,  # noqa: F401
                                  _component_counts, _iou_records, _mesh_records, _mesh_stats_records, _mesh_stats_rows, _normal_records,
                                  _write_mesh_stats_lines, iou_line, mesh_stats_line)

try:
    from ..utils import util_vis
except Exception:  # pragma: no cover
    util_vis = None


def _rank0(opt):
    if opt.get("rank", None) is not None:      # set by the launcher when ranks and device indices are numbered differently
        return int(opt.rank) == 0
    return opt.device == 0 or opt.device in ("cuda:0", "cpu")


def _train_vis(opt):
    """`--hip.train_vis` (default off): the reference's training-time visualisation on rank 0 -- the visualisation samples, vis_log/iter_{it}/
    every freq.save_vis iterations and vis_{ep}/ (PNGs, mesh, point cloud, turn-table GIFs) at every training-time evaluation."""
    return bool(options.hip(opt, "train_vis")) and _rank0(opt)


def _mesh_color(opt):
    """`--hip.mesh_color` (default off): every mesh dump also writes {idx}_mesh_color.ply, the same mesh with per-vertex normals and
    predicted colours (eval_3D.mesh_attributes)."""
    return bool(options.hip(opt, "mesh_color"))


def _surface_render(opt):
    """`--hip.surface_render` (default off): every per-sample dump also gets the sharp surface render of the sample's view
    (Renderer.render_surface with `--hip.surface_refine` rounds at `--hip.surface_scale` times the evaluation resolution):
    {idx}_image_surface.png, _mask_surface.png, _normal_surface.png, _depth_surface.png and _depth_surface.npy."""
    return bool(options.hip(opt, "surface_render"))


class Runner:

    def __init__(self, opt):
        if os.path.isdir(opt.output_path) and opt.resume is False and _rank0(opt):
            for fn in os.listdir(opt.output_path):
                if "tfevents" in fn:
                    os.remove(os.path.join(opt.output_path, fn))
                if "vis" in fn:
                    shutil.rmtree(os.path.join(opt.output_path, fn), ignore_errors=True)
        if _rank0(opt):
            os.makedirs(opt.output_path, exist_ok=True)
        if "world_size" not in opt:
            opt.world_size = 1
        if opt.world_size > 1 and not torch.distributed.is_initialized():
            setup(opt.device, opt.world_size, opt.port)
        opt.batch_size = opt.batch_size // opt.world_size
        self.optimizer = getattr(torch.optim, opt.optim.algo)
        self.tb = None
        self.reducer = None

    # ---- data -----------------------------------------------------------------------------------------
    def load_dataset(self, opt, eval_split="val"):
        data = importlib.import_module("data.{}".format(opt.data.dataset))
        if _rank0(opt): log.info("loading training data...")
        self.train_data = data.Dataset(opt, split="train")
        self.train_loader = self.train_data.setup_loader(opt, shuffle=True)
        self.num_batches = len(self.train_loader)
        if _rank0(opt): log.info("loading test data...")
        self.test_data = data.Dataset(opt, split=eval_split)
        self.test_loader = self.test_data.setup_loader(opt, shuffle=False, drop_last=False, batch_size=opt.eval.batch_size)
        self.viz_data = []
        if _train_vis(opt):
            # reference runner.py:105-111: a shuffled loader over the evaluation split, iterated here -- its sampler draws from the CPU
            # generator, which is why nothing of this runs without --hip.train_vis
            log.info("creating data for visualization...")
            self.viz_loader = self.test_data.setup_loader(opt, shuffle=True, drop_last=False, batch_size=opt.eval.batch_size)
            self.viz_loader_iter = iter(self.viz_loader)
            for _ in range(opt.eval.n_vis):
                self.append_viz_data(opt)

    def append_viz_data(self, opt):
        """One sample per category from the visualisation loader until n_vis_classes categories are covered (reference runner.py:60-89);
        each sample is kept as a batch of one (its tensors [1, ...], nested dictionaries likewise)."""
        cat_samples = [0] * opt.data.num_classes
        n_vis_classes = min(opt.eval.n_vis_classes if "n_vis_classes" in opt.eval else opt.data.num_classes, opt.data.num_classes)
        while sum(cat_samples) < n_vis_classes:
            batch = next(self.viz_loader_iter)
            for i, cat in enumerate(batch["category_label"]):
                c = int(cat)
                if cat_samples[c] >= 1:
                    continue
                cat_samples[c] += 1
                sample = {}
                for key, value in batch.items():
                    if isinstance(value, torch.Tensor):
                        sample[key] = value[i].unsqueeze(0)
                    elif isinstance(value, dict):
                        sample[key] = {k: v[i].unsqueeze(0) for k, v in value.items()}
                    else:
                        raise NotImplementedError(key)
                self.viz_data.append(sample)

    # ---- networks / optimisers ------------------------------------------------------------------------
    def build_networks(self, opt):
        if _rank0(opt): log.info("building networks...")
        name = "pretrainer" if opt.pretrain else "graph"
        module = importlib.import_module("shapeclipper_amd.model.{}".format(name))
        dev = torch.device("cuda", opt.device) if isinstance(opt.device, int) else torch.device(opt.device)
        # `--hip.reserve_cus=N` (default 0): in a multi-GPU step the persistent one-workgroup-per-CU grids of the trunk convolutions are sized
        # for (CUs - N), leaving N compute units to RCCL's all-reduce kernels.  Set before any workspace is sized;
        # single-GPU runs keep every CU.
        reserve = int(options.hip(opt, "reserve_cus") or 0)
        if dev.type == "cuda":
            from .. import ops
            ops.set_reserved_cus(reserve if opt.world_size > 1 else 0)
        self.graph = ModuleHolder(module.Graph(opt).to(dev))
        if opt.world_size > 1:
            # Default (round 4): north_star's SINGLE flat all-reduce after backward.  `--hip.overlap_allreduce` lays the buffer out
            # [early 94.5 % | late] and issues the early segment from inside backward on a side stream; on one rank its hooks and stream
            # juggling cost 1.1 ms of host time per step more than the single collective (profiles/r04_overlap_1rank.txt) on a step that
            # is host-paced, against ~0.7-1 ms of xGMI time it could hide: not the default until a multi-GPU run says otherwise.
            self.reducer = FlatGradAllReduce(self.graph.module, opt.world_size,
                                             overlap=None if options.hip(opt, "overlap_allreduce") else False)

    def setup_optimizer(self, opt):
        if _rank0(opt): log.info("setting up optimizers...")
        kwargs = {k: (tuple(v) if k == "betas" else v) for k, v in opt.optim.params.items()}
        on_gpu = next(self.graph.parameters()).is_cuda
        if on_gpu and self.optimizer in (torch.optim.Adam, torch.optim.AdamW) and options.hip(opt, "fused_adam"):
            kwargs.setdefault("fused", True)       # one multi-tensor kernel instead of ~90 foreach launches per step
        full, view = [], []
        for k, v in self.graph.named_parameters():
            full.append(v)
            if "estimator" in k:
                view.append(v)
        self.optim_full = self.optimizer([dict(params=full, lr=opt.optim.lr)], **kwargs)
        self.optim_V = self.optimizer([dict(params=view, lr=opt.optim.lr)], **kwargs)
        # hip.guarded_step: the fused optimizer takes the step's NaN / Inf flag as its `found_inf` tensor (the hook torch's GradScaler uses) and
        # skips the update ON THE DEVICE; the host then reads the flag one step late instead of waiting for it before every optim.step()
        self._guarded_step = bool(kwargs.get("fused")) and bool(options.hip(opt, "guarded_step"))

    def restore_checkpoint(self, opt, best=False, evaluate=False):
        epoch_start, iter_start = None, None
        if opt.resume:
            if _rank0(opt): log.info("resuming from previous checkpoint...")
            epoch_start, iter_start, self.best_val = util.restore_checkpoint(
                opt, self, resume=opt.resume, best=best if opt.data.dataset != "openimage" else False, evaluate=evaluate)
        elif opt.load is not None:
            if _rank0(opt): log.info("loading weights from checkpoint {}...".format(opt.load))
            epoch_start, iter_start, _ = util.restore_checkpoint(opt, self, load_name=opt.load)
        elif _rank0(opt):
            log.info("initializing weights from scratch...")
        self.epoch_start = epoch_start or 0
        self.iter_start = iter_start or 0

    def setup_visualizer(self, opt):
        if _rank0(opt) and opt.tb:
            try:
                from torch.utils.tensorboard import SummaryWriter
                self.tb = SummaryWriter(log_dir=opt.output_path, flush_secs=10)
            except Exception:
                log.info("tensorboard not available; scalar logging goes to stdout only")

    # ---- training -------------------------------------------------------------------------------------
    def train(self, opt):
        if _rank0(opt): log.title("TRAINING START")
        self.graph.module.estimator.reset_scales()
        self.timer = edict(start=time.time(), it_mean=None)
        self.iter_skip = self.iter_start % len(self.train_loader)
        self.it = self.iter_start
        if not opt.resume:
            self.best_val, self.best_ep = np.inf, 1
        if self.iter_start == 0 and _rank0(opt) and opt.freq.eval:
            self.evaluate(opt, ep=0, training=True)
        for self.ep in range(self.epoch_start, opt.max_epoch):
            self.train_epoch(opt)
        if _rank0(opt):
            self.save_checkpoint(opt, ep=self.ep + 1, it=self.it, best_val=self.best_val)
            if self.tb is not None:
                self.tb.flush(); self.tb.close()
            log.title("TRAINING DONE")
            log.info("Best CD: %.4f @ epoch %d" % (self.best_val, self.best_ep))
        if opt.world_size > 1:
            cleanup()

    def train_epoch(self, opt):
        if opt.world_size > 1:
            torch.distributed.barrier()
            if hasattr(self.train_loader, "sampler") and hasattr(self.train_loader.sampler, "set_epoch"):
                self.train_loader.sampler.set_epoch(self.ep)
        progress = tqdm.tqdm(range(self.num_batches), desc="training epoch {}".format(self.ep + 1), leave=False) \
            if _rank0(opt) else range(self.num_batches)
        self.graph.train()
        loader = iter(self.train_loader)
        loss = None
        for _ in progress:
            if self.iter_skip > 0:          # fast-forward after --resume
                self.iter_skip -= 1
                continue
            var = edict(next(loader))
            opt.H, opt.W = opt.image_size
            var = util.move_to_device(var, opt.device)
            var = sample_rays_device(opt, var)        # Pix3D batches with ray_seed (hip.device_rays): silhouette rays drawn on the device
            loss = self.train_iteration(opt, var, progress)
        self.check_finite()                   # the last iteration's deferred NaN/Inf check
        if _rank0(opt) and loss is not None:
            log.loss_train(opt, self.ep + 1, opt.optim.lr, loss, self.timer)
        if (self.ep + 1) % opt.freq.eval == 0 and _rank0(opt):
            val = self.evaluate(opt, ep=self.ep + 1, training=True)
            if val < self.best_val:
                self.best_val, self.best_ep = val, self.ep + 1
                self.save_checkpoint(opt, ep=self.ep + 1, it=self.it, best_val=self.best_val, best=True, latest=True)

    def train_iteration(self, opt, var, loader=None):
        self.timer.it_start = time.time()
        frozen_keys = []
        if self.it > opt.optim.iter_camera:
            optim = self.optim_full
        else:                                  # camera warm-up: only the estimator learns
            for m in self.graph.modules():
                if isinstance(m, torch.nn.BatchNorm2d):
                    m.eval()
            optim = self.optim_V
            frozen_keys = ["nearest_img", "nearest_mask", "nearest_normal", "eikonal"]
        if self.reducer is not None:
            self.reducer.zero_grad()
            self.reducer.broadcast_buffers()
        else:
            optim.zero_grad()
        var, loss = self.graph.forward(opt, var, training=True, get_loss=True)
        loss = self.summarize_loss(opt, var, loss, non_act_loss_key=frozen_keys, defer_check=True)
        loss.all.backward()
        if self.reducer is not None:
            self.reducer.all_reduce()
        # The reference asserts on NaN / Inf losses before it back-propagates (runner.py:296-302).  Here the flag left for pinned memory
        # right after the forward pass.  Guarded step (default with the fused optimizer): the flag is also the optimizer's `found_inf`, so a
        # poisoned step leaves the weights, the Adam moments and the step counters untouched without the host knowing yet; the host reads
        # the flag of the PREVIOUS step here (complete long ago: no wait -- the per-step wait cost 1.0 ms of 36.6 at bs32, 0.3 of 22.0 at
        # bs16, measured round 4 with tools/step_times.py) and raises the reference's assertion one step late, before this step's update is applied.
        # Otherwise (foreach / CPU optimizers): wait for this step's flag now, before optim.step().
        if getattr(self, "_guarded_step", False):
            optim.grad_scale, optim.found_inf = None, getattr(self, "_step_found_inf", None)
            self.check_finite(keep_last=True)
        else:
            self.check_finite()
        optim.step()

        # Never checkpoint a step whose losses were not verified -- and EVERY rank drains its pending flags at a checkpoint iteration, not
        # only rank 0: the flag is MAX-reduced over the ranks, so all of them raise here together instead of rank 0 dying alone
        # and the others walking into the next step's collectives against a dead peer.
        if (self.it + 1) % opt.freq.ckpt_latest == 0:
            self.check_finite()
        if _rank0(opt):
            if (self.it + 1) % opt.freq.ckpt_latest == 0:
                self.save_checkpoint(opt, ep=self.ep, it=self.it + 1, best_val=self.best_val, latest=True)
            if opt.freq.scalar and self.it % opt.freq.scalar == 0 and self.tb is not None:
                self.log_scalars(opt, var, loss, step=self.it, split="train")
                self.tb.add_scalar("train/beta", self.graph.module.renderer.density.beta, global_step=self.it)
            if _train_vis(opt) and opt.freq.save_vis and self.it % opt.freq.save_vis == 0:
                self.save_vis(opt)
        self.it += 1
        if loader is not None and hasattr(loader, "set_postfix") and self.it % 10 == 0:
            loader.set_postfix(it=self.it, loss="{:.3f}".format(float(loss.all)))
        self.timer.it_end = time.time()
        util.update_timer(opt, self.timer, self.ep if hasattr(self, "ep") else 0, len(loader) if loader is not None else 1)
        return loss

    def summarize_loss(self, opt, var, loss, non_act_loss_key=[], defer_check=False):
        """all = sum_k float(w_k) * loss_k (keys in non_act_loss_key weigh 0).  NaN/Inf are checked with ONE
        host read of a device flag instead of two syncs per key (reference runner.py:296-302).  With defer_check the
        flag travels to pinned host memory asynchronously and `check_finite(loss)` raises the same assertions later
        (train_iteration calls it after the backward pass is queued and before the optimizer step)."""
        assert "all" not in loss
        total, bad = 0., None
        keys = []
        for key in loss:
            assert key in opt.loss_weight
            if opt.loss_weight[key] is not None:
                keys.append(key)
        weights = tuple(0.0 if key in non_act_loss_key else float(opt.loss_weight[key]) for key in keys)
        values = [loss[key] if loss[key].dim() == 0 else loss[key].mean() for key in keys]
        from .. import ops
        if values and all(v.is_cuda for v in values) and len(values) <= ops.LOSS_TOTAL_MAX_TERMS:
            # the weighted sum (same order of additions) and the NaN/Inf flag of every term in one launch (csrc/camera_prior.hip)
            from ..functional import LossTotalFunction
            total, bad = LossTotalFunction.apply(weights, *values)
        else:
            for w, value in zip(weights, values):
                flag = ~torch.isfinite(value)
                bad = flag if bad is None else (bad | flag)
                total = total + w * value
        if "_bad_choice" in var and bad is not None:          # NaN neighbour probabilities (np.random.choice would have raised)
            bad = bad | var.pop("_bad_choice").to(bad.device)
        self._step_found_inf = None
        if bad is not None and opt.get("check_finite", True):
            reducer = getattr(self, "reducer", None)
            if defer_check and reducer is not None and reducer.comm:
                # multi-rank: MAX of the flag over the ranks, so that every rank raises (or none does) before optim.step()
                flag = reducer.reduce_flag(bad)
                stream = reducer._comm_stream
                if flag.is_cuda:
                    host = torch.empty((1,), dtype=torch.float32, pin_memory=True)
                    with torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext():
                        host.copy_(flag, non_blocking=True)
                        done = torch.cuda.Event()
                        done.record()
                    self._pending().append((host, done, {k: v.detach() for k, v in loss.items()}))
                    self._step_found_inf = flag.reshape(())  # exactly 1.0 where any rank's loss is NaN / Inf (MAX of 0 / 1 flags)
                elif bool(flag.item() > 0):
                    self._raise_not_finite(loss, any_rank=True)
            elif defer_check and bad.is_cuda:
                host = torch.empty((), dtype=torch.bool, pin_memory=True)
                host.copy_(bad, non_blocking=True)
                done = torch.cuda.Event()
                done.record()
                self._pending().append((host, done, {k: v.detach() for k, v in loss.items()}))
                self._step_found_inf = bad.detach().reshape(()).to(torch.float32)      # 0-dim, as GradScaler's
            elif bool(bad):
                self._raise_not_finite(loss)
        loss.update(all=total)
        return loss

    @staticmethod
    def _raise_not_finite(loss, any_rank=False):
        for key in loss:
            if key == "all":
                continue
            v = loss[key].mean()
            assert not torch.isinf(v), "loss {} is Inf".format(key)
            assert not torch.isnan(v), "loss {} is NaN".format(key)
        # multi-rank: the flag is the MAX over the ranks -- this rank's losses are finite, another rank's are not; every rank stops here
        assert not any_rank, "a loss is NaN / Inf on another rank"

    def _pending(self):
        if not hasattr(self, "_pending_checks"):
            self._pending_checks = []
        return self._pending_checks

    def check_finite(self, loss=None, keep_last=False):
        """Raise the reference's NaN/Inf assertions (runner.py:296-302) for the steps whose flags are pending, oldest first.
        train_iteration calls this between the (queued) backward pass and the optimizer step: each flag was copied to pinned memory
        right after its forward pass.  keep_last (guarded step): the newest flag stays pending -- its step is protected on the device
        by the optimizer's `found_inf` -- so the wait is for the previous step's event, which completed long ago.  Without keep_last
        (end of an epoch, before a checkpoint, unguarded optimizers) every pending flag is waited for."""
        queue = self._pending()
        while len(queue) > (1 if keep_last else 0):
            host, done, pending_loss = queue.pop(0)
            done.synchronize()
            if bool(host.reshape(-1)[0] > 0):
                queue.clear()
                self._raise_not_finite(loss if loss is not None else pending_loss, any_rank=host.dtype != torch.bool)

    # ---- evaluation -----------------------------------------------------------------------------------
    @torch.no_grad()
    def evaluate(self, opt, ep, training=False):
        self.graph.eval()
        opt.H, opt.W = opt.eval.image_size
        f_scores = []
        metric = dict(dist_acc=0., dist_cov=0.)
        C = opt.data.num_classes
        acc_cat, comp_cat, counts = [0.] * C, [0.] * C, [0.001] * C
        f_scores_icp, acc_cat_icp, comp_cat_icp = [], [0.] * C, [0.] * C     # --eval.icp: the same tallies of the ICP-aligned metrics
        tabled = [rep for rep in REPORTS if rep.base.tables]                 # dump_results writes the per-sample lines of every report
        recs = {rep.key: [] for rep in tabled}                               # the records of every batch, for the per-category tables
        loader = tqdm.tqdm(self.test_loader, desc="evaluating", leave=False)
        for it, batch in enumerate(loader):
            var = self.evaluate_batch(opt, edict(batch), ep, it, single_gpu=True)
            dist_acc, dist_cov = eval_3D.eval_metrics(opt, var, self.graph.module.sdf_network)
            f_scores.append(var.f_score)
            for i in range(len(var.idx)):
                c = var.category_label[i].item()
                counts[c] += 1; acc_cat[c] += var.cd_acc[i].item(); comp_cat[c] += var.cd_comp[i].item()
                if "icp" in var:
                    acc_cat_icp[c] += var.cd_acc_icp[i].item(); comp_cat_icp[c] += var.cd_comp_icp[i].item()
            if "icp" in var:
                f_scores_icp.append(var.f_score_icp)
            for rep in tabled:
                if rep.present(var, opt):
                    recs[rep.key].append(rep.records(var))
            metric["dist_acc"] += dist_acc * len(var.idx)
            metric["dist_cov"] += dist_cov * len(var.idx)
            loader.set_postfix(CD="{:.3f}".format(float((dist_acc + dist_cov) / 2)))
            if it == 0 and training and _train_vis(opt):
                self.visualize_samples(opt, ep)
            if not training:
                self.dump_results(opt, var, ep, write_new=(it == 0))
        if not training:
            names = self._category_names(opt)
            with open(os.path.join(opt.output_path, "cd_cat.txt"), "w") as f:
                f.write("CD     Acc    Comp   Count Cat\n")
                for i in range(C):
                    a, c = acc_cat[i] / counts[i], comp_cat[i] / counts[i]
                    f.write("%.4f %.4f %.4f %5d %s\n" % ((a + c) / 2, a, c, counts[i], names[i]))
            fs = torch.cat(f_scores, dim=0).mean(dim=0)
            with open(os.path.join(opt.output_path, "f_score.txt"), "w") as f:
                for i, th in enumerate(opt.eval.f_thresholds):
                    line = "F-score @ %.2f: %.4f" % (th * 100, fs[i].item())
                    print(line); f.write(line + "\n")
            if f_scores_icp:                            # cd_cat_icp.txt / f_score_icp.txt, in the formats of their namesakes
                with open(os.path.join(opt.output_path, "cd_cat_icp.txt"), "w") as f:
                    f.write("CD     Acc    Comp   Count Cat\n")
                    for i in range(C):
                        a, c = acc_cat_icp[i] / counts[i], comp_cat_icp[i] / counts[i]
                        f.write("%.4f %.4f %.4f %5d %s\n" % ((a + c) / 2, a, c, counts[i], names[i]))
                fs = torch.cat(f_scores_icp, dim=0).mean(dim=0)
                with open(os.path.join(opt.output_path, "f_score_icp.txt"), "w") as f:
                    for i, th in enumerate(opt.eval.f_thresholds):
                        f.write("F-score @ %.2f: %.4f\n" % (th * 100, fs[i].item()))
            for rep in tabled:
                if recs[rep.key]:
                    self._write_report(opt, torch.cat(recs[rep.key]), per_sample=False, key=rep.key)
        n = max(len(self.test_data), 1)
        for k in metric:
            metric[k] /= n
        log.loss_eval(opt, loss=None, chamfer=(metric["dist_acc"], metric["dist_cov"]))
        opt.H, opt.W = opt.image_size
        return float((metric["dist_acc"] + metric["dist_cov"]) / 2)

    @torch.no_grad()
    def evaluate_sharded(self, opt, ep=0):
        """Evaluation over all ranks (BASELINE config[4]; the reference evaluates on one GPU, evaluate.py:16-18): rank r takes the test
        samples with index % world == r (eval.batch_size = 1), the per-sample records are gathered, and rank 0 writes chamfer.txt /
        cd_cat.txt / f_score.txt in sample order.  Every optional output that is enabled (eval_reports.REPORTS, in that order) costs one
        more gather of its records, which every rank joins, also one that evaluated no sample; rank 0 writes its files.  The value
        returned is the raw one.  Every rank writes the per-sample files of its own samples (dump_visuals: PNGs, mesh and point-cloud PLYs)."""
        from ..parallel import gather_eval_records
        self.graph.eval()
        opt.H, opt.W = opt.eval.image_size
        # the reference's single-node convention is rank == device index; the process group's rank is the same number there and stays
        # right when ranks and devices are numbered differently (several nodes; tests/test_gpu_two_ranks.py: two ranks on one GPU)
        rank = torch.distributed.get_rank() if torch.distributed.is_initialized() else util.get_rank(opt)
        raw, recs = [], {rep.key: [] for rep in REPORTS}
        for it in range(rank, len(self.test_data), opt.world_size):
            sample = self.test_data[it]
            batch = {k: ({kk: vv[None] for kk, vv in v.items()} if isinstance(v, dict) else torch.as_tensor(v)[None]) for k, v in sample.items()}
            var = self.evaluate_batch(opt, edict(batch), ep, it, single_gpu=True)
            eval_3D.eval_metrics(opt, var, self.graph.module.sdf_network)
            self.dump_visuals(opt, var, ep)             # this rank's samples only (dump_geometry leaves var.texture / var.mesh_render)
            raw.append(torch.cat([var.idx.float().view(1), var.cd_acc.view(1), var.cd_comp.view(1), var.f_score.view(-1),
                                  var.category_label.float().view(1)]))
            for rep in REPORTS:
                if rep.present(var, opt):
                    recs[rep.key].append(rep.records(var))
        dev = next(self.graph.parameters()).device
        records = torch.stack(raw) if raw else torch.zeros(0, 10, device=dev)
        allr = gather_eval_records(records.to(dev), opt.world_size).cpu()
        gathered = {}
        for rep in REPORTS:
            if rep.enabled(opt):
                mine = torch.cat(recs[rep.key]) if recs[rep.key] else torch.zeros(0, rep.width(opt), dtype=torch.float64)
                gathered[rep.key] = gather_eval_records(mine.to(dev), opt.world_size).cpu()
        opt.H, opt.W = opt.image_size
        if rank == 0:
            for key, rows in gathered.items():
                self._write_report(opt, rows, key=key)
            if "icp" in gathered:                       # the metrics are fp32 values: tallied as the raw records are
                self._write_gathered(opt, gathered["icp"][:, :REPORT["icp"].layout(opt)[ICP_KEYS[0]]].float(), "_icp")
            self._write_gathered(opt, allr)
            log.loss_eval(opt, loss=None, chamfer=(allr[:, 1].mean(), allr[:, 2].mean()))
        return float((allr[:, 1].mean() + allr[:, 2].mean()) / 2) if allr.shape[0] else float("nan")

    def _category_names(self, opt):
        return getattr(self.test_data, "label2cat", {i: str(i) for i in range(opt.data.num_classes)})


    def _write_gathered(self, opt, allr, suffix=""):
        """chamfer{suffix}.txt, cd_cat{suffix}.txt and f_score{suffix}.txt from gathered records [N,10] = (idx, cd_acc, cd_comp, f_score[6],
        category) in sample order: the raw metrics (suffix "") and, with --eval.icp, the ICP-aligned ones ("_icp")."""
        with open("{}/chamfer{}.txt".format(opt.output_path, suffix), "w") as f:
            for r in allr:
                f.write("{} {:.8f} {:.8f}\n".format(int(r[0]), r[1], r[2]))
        C = opt.data.num_classes
        names = getattr(self.test_data, "label2cat", {i: str(i) for i in range(C)})
        with open(os.path.join(opt.output_path, "cd_cat{}.txt".format(suffix)), "w") as f:
            f.write("CD     Acc    Comp   Count Cat\n")
            for c in range(C):
                sel = allr[allr[:, 9] == c]
                n = sel.shape[0] + 0.001
                a_, c_ = float(sel[:, 1].sum()) / n, float(sel[:, 2].sum()) / n
                f.write("%.4f %.4f %.4f %5d %s\n" % ((a_ + c_) / 2, a_, c_, n, names[c]))
        fs = allr[:, 3:9].mean(dim=0)
        with open(os.path.join(opt.output_path, "f_score{}.txt".format(suffix)), "w") as f:
            for i, th in enumerate(opt.eval.f_thresholds):
                f.write("F-score @ %.2f: %.4f\n" % (th * 100, fs[i].item()))

    def _write_report(self, opt, rows, per_sample=True, key=None):
        """The files of one report from its records in sample order (eval_reports.Report.write)."""
        REPORT[key].write(opt, rows, Runner._category_names(self, opt), per_sample)

    _write_normals = functools.partialmethod(_write_report, key="normals")
    _write_mesh = functools.partialmethod(_write_report, key="mesh_dist")
    _write_iou = functools.partialmethod(_write_report, key="iou")
    _write_mesh_stats = functools.partialmethod(_write_report, key="mesh_stats")

    def evaluate_batch(self, opt, var, ep=None, it=None, single_gpu=False, visualize=False):
        var = util.move_to_device(var, opt.device)
        return self.graph.module(opt, var, training=False, visualize=visualize, get_loss=False)

    @torch.no_grad()
    def save_vis(self, opt):
        """vis_log/iter_{it}/: the seven PNGs of every visualisation sample (reference runner.py:267-286, every freq.save_vis iterations)."""
        opt.H, opt.W = opt.eval.image_size
        self.graph.eval()
        folder = "vis_log/iter_{}".format(self.it)
        os.makedirs("{}/{}".format(opt.output_path, folder), exist_ok=True)
        for sample in self.viz_data:
            var = util.move_to_device(edict(deepcopy(sample)), opt.device)
            var = self.graph.module(opt, var, training=False, visualize=False, get_loss=False)
            if "normal_input_map" not in var:
                var.normal_input_map = var.normal_gt.view(len(var.idx), opt.image_size[0], opt.image_size[1], 3).permute(0, 3, 1, 2).contiguous()
            self.dump_vis_images(opt, var, folder, input_pose=False)
        opt.H, opt.W = opt.image_size
        self.graph.train()

    @torch.no_grad()
    def visualize_samples(self, opt, ep, n_views=50):
        """vis_{ep}/ of every visualisation sample: the `it == 0 and training` block of the reference's evaluate (runner.py:349-357) without
        its TensorBoard grids -- the visualize=True render, the n_views turn-table (batched on the HIP chain), the mesh and the dumps."""
        renderer = self.graph.module.renderer
        batched = not renderer.eager and opt.camera.model == "perspective"
        for n, sample in enumerate(self.viz_data):
            var = self.evaluate_batch(opt, edict(deepcopy(sample)), ep, 0, single_gpu=True, visualize=True)
            var = self.graph.module.get_rotate_pose(opt, var, n_views=n_views)
            self.vis_rotate(opt, var, n_views=n_views, batched=batched)
            eval_3D.eval_metrics(opt, var, self.graph.module.sdf_network, vis_only=True)
            self.dump_train_vis(opt, var, ep)
            if "mesh_stats" in var:                     # --eval.mesh_stats: vis_{ep}/mesh_stats.txt of the visualised samples
                _write_mesh_stats_lines("{}/vis_{}".format(opt.output_path, ep), _mesh_stats_records(var), "w" if n == 0 else "a")

    @torch.no_grad()
    def vis_rotate(self, opt, var, n_views=50, vis_NN=False, batched=False, chunk_views=None):
        """The turn-table of reference runner.py:406-427: var.rotating_imgs / rotating_masks / rotating_normals, n_views lists of [B,c,H,W]
        maps (normals / 2 + 0.5).  batched=False renders the views one after another, the reference's loop.  batched=True makes the same
        draws of the random generator first (each view's render draws its eikonal sample indices, unused at training=False) and renders
        every view in as few passes of the HIP chain as memory allows (Renderer.render_views; chunk_views views per pass when given):
        bit-identical maps, and the per-ray outputs stay in var.rotating_raw = (rgb, mask, normal) [n_views,B,R,c] for ops.vis_frames."""
        B = len(var.idx)
        renderer = self.graph.module.renderer
        latent_rgb = var.proj_latent_rgb_NN if vis_NN else var.proj_latent_rgb
        if batched:
            rdev = var.intr.device if options.hip(opt, "device_rng") else "cpu"
            for _ in range(n_views):
                torch.randint(renderer.N_samples, (B * opt.H * opt.W,), device=rdev)
            rgb, mask, normal = renderer.render_views(opt, var.vis_pose[:n_views], var.intr, var.proj_latent_sdf, latent_rgb,
                                                      chunk_views=chunk_views)
            maps = lambda x: [m.view(B, opt.H, opt.W, -1).permute(0, 3, 1, 2) for m in x.unbind(0)]
            var.rotating_imgs, var.rotating_masks, var.rotating_normals = maps(rgb), maps(mask), maps(normal / 2 + 0.5)
            var.rotating_raw = (rgb, mask, normal)
            return
        imgs, masks, normals = [], [], []
        as_map = lambda x, c: x.view(B, opt.H, opt.W, c).permute(0, 3, 1, 2).contiguous()
        for i in range(n_views):
            pose_i = var.vis_pose[i].unsqueeze(0).expand(B, -1, -1)
            rgb, mask, _, _, normal, _ = renderer(opt, pose_i, var.intr, torch.ones_like(var.scale_dist), var.proj_latent_sdf, latent_rgb,
                                                  training=False)
            imgs.append(as_map(rgb, 3)); masks.append(as_map(mask, 1)); normals.append(as_map(normal, 3) / 2 + 0.5)
        var.rotating_imgs, var.rotating_masks, var.rotating_normals = imgs, masks, normals

    @torch.no_grad()
    def log_scalars(self, opt, var, loss, metric=None, step=0, split="train"):
        if self.tb is None:
            return
        for key, value in loss.items():
            if key != "all":
                self.tb.add_scalar("{0}/loss_{1}".format(split, key), value.mean(), step)
        for key, value in (metric or {}).items():
            self.tb.add_scalar("{0}/{1}".format(split, key), value, step)

    @torch.no_grad()
    def dump_visuals(self, opt, var, ep, train=False):
        """Per-sample files of an evaluated batch: the two PNGs and, outside training, {idx}_mesh.ply (the predicted mesh) and
        {idx}_pointclouds_comp.ply (the points eval_metrics compared: prediction red, ground truth green).  File names carry the
        sample index, so the ranks of evaluate_sharded never write the same file."""
        folder = "dump" if not train else "vis_{}".format(ep)
        os.makedirs("{}/{}/".format(opt.output_path, folder), exist_ok=True)
        if util_vis is None:
            return
        util_vis.dump_images(opt, var.idx, "image_recon", var.rgb_recon_map, masks=var.mask_hard_map, folder=folder)
        util_vis.dump_images(opt, var.idx, "mask_recon", var.mask_recon_map, folder=folder)
        if train:
            return
        self.dump_geometry(opt, var, folder)
        if _surface_render(opt):
            self.dump_surface(opt, var, folder)

    @torch.no_grad()
    def dump_vis_images(self, opt, var, folder, input_pose=True):
        """The PNGs of a visualisation sample (reference dump_results, runner.py:473-482): input and reconstruction with the pose axes drawn
        (the input's only when input_pose), masks, and the input, canonical and reconstructed normals."""
        if util_vis is None:
            return
        dump = lambda name, images, **kw: util_vis.dump_images(opt, var.idx, name, images, folder=folder, **kw)
        dump("image_input", var.rgb_input_map, poses=var.get("pose_gt") if input_pose else None)
        dump("image_recon", var.rgb_recon_map, masks=var.mask_hard_map, poses=var.pose)
        dump("mask_recon", var.mask_recon_map)
        dump("mask_input", var.mask_input_map)
        for name, key in (("normal_input_viewpoint", "normal_input_map"), ("normal_input_canonical", "normal_transformed_map"),
                          ("normal_recon", "normal_recon_map")):
            if key in var:
                dump(name, var[key], from_range=(-1, 1))

    @torch.no_grad()
    def dump_train_vis(self, opt, var, ep):
        """vis_{ep}/ of a visualisation sample (reference dump_results(train=True), runner.py:469-497): the PNGs, {idx}_mesh.ply,
        {idx}_pointclouds_comp.ply and the rotating GIFs {idx}_image_rotate.gif, _mask_rotate.gif, _normal_rotate.gif."""
        folder = "vis_{}".format(ep)
        os.makedirs("{}/{}/".format(opt.output_path, folder), exist_ok=True)
        if util_vis is None:
            return
        self.dump_vis_images(opt, var, folder)
        self.dump_geometry(opt, var, folder)
        for name, frames in self.turntable_frames(opt, var).items():
            util_vis.dump_gifs(opt, var.idx, name, frames, folder=folder)
        if options.mesh_render(opt) and "vis_pose" in var:
            self.dump_mesh_turntable(opt, var, folder)
        if _surface_render(opt):
            self.dump_surface(opt, var, folder, rotate=True)

    @staticmethod
    def turntable_frames(opt, var):
        """{gif name: uint8 frames [B, n_views, H, W, 3]} of var's turn-table, by ops.vis_frames: from the per-ray outputs of the batched
        turn-table (var.rotating_raw), else from the maps of the per-view loop (whose normals are already / 2 + 0.5)."""
        from .. import ops
        B = len(var.idx)
        if "rotating_raw" in var:
            outs, kinds = var.rotating_raw, ("rgb", "mask", "normal")
        else:
            stack = lambda maps: torch.stack(maps).permute(0, 1, 3, 4, 2)          # [V,B,c,H,W] -> [V,B,H,W,c]
            outs, kinds = (stack(var.rotating_imgs), stack(var.rotating_masks), stack(var.rotating_normals)), ("rgb", "mask", "rgb")
        return {name: ops.vis_frames(x.reshape(x.shape[0], B, opt.H, opt.W, -1), kind).transpose(0, 1)
                for name, x, kind in zip(("image_rotate", "mask_rotate", "normal_rotate"), outs, kinds)}

    @torch.no_grad()
    def dump_surface(self, opt, var, folder, rotate=False):
        """The files of `--hip.surface_render` for an evaluated batch, k = hip.surface_scale times opt.H x opt.W pixels each:
        {idx}_image_surface.png (predicted colour at the surface point, data.bgcolor where the ray misses), {idx}_mask_surface.png (1 where
        the ray meets the solid {sdf < 0}), {idx}_normal_surface.png (the unit normal in the encoding of the other normal PNGs,
        (n + 1) / 2; misses are mid-grey), {idx}_depth_surface.png (Renderer.surface_depth_grey: black at the near sample plane, white at
        the far one and where the ray misses) and {idx}_depth_surface.npy (the raw fp32 depth [k H, k W], 0 where the ray misses).
        rotate=True (the vis_{ep}/ dump of --hip.train_vis): also {idx}_image_surface_rotate.gif and {idx}_normal_surface_rotate.gif, the
        surface render from every pose of var.vis_pose (Renderer.render_views(surface=True), frames by ops.vis_frames).
        The surface render shows the raw network: --hip.largest_component filters the level grid, not the MLP.  var.surface keeps the
        SurfaceRender as a dict."""
        if util_vis is None:
            return
        from .. import ops
        k, n_refine = int(options.hip(opt, "surface_scale")), int(options.hip(opt, "surface_refine"))
        renderer = self.graph.module.renderer
        B, H, W = len(var.idx), k * opt.H, k * opt.W
        out = renderer.render_surface(opt, var.pose, var.intr, var.scale_dist, var.proj_latent_sdf, var.proj_latent_rgb, n_refine=n_refine, scale=k)
        var.surface = out._asdict()
        as_map = lambda x: x.view(B, H, W, -1).permute(0, 3, 1, 2)
        grey = renderer.surface_depth_grey(opt, out, var.pose, var.intr, var.scale_dist, scale=k)
        dump = lambda name, images, **kw: util_vis.dump_images(opt, var.idx, name, images, folder=folder, **kw)
        dump("image_surface", as_map(out.rgb))
        dump("mask_surface", as_map(out.mask))
        dump("normal_surface", as_map(out.normal), from_range=(-1, 1))
        dump("depth_surface", as_map(grey))
        util_vis.dump_arrays(opt, var.idx, "depth_surface", out.depth.view(B, H, W), folder=folder)
        if rotate and "vis_pose" in var:
            views = renderer.render_views(opt, var.vis_pose, var.intr, var.proj_latent_sdf, var.proj_latent_rgb, surface=True,
                                          n_refine=n_refine, scale=k)
            for name, x, kind in (("image_surface_rotate", views.rgb, "rgb"), ("normal_surface_rotate", views.normal, "normal")):
                frames = ops.vis_frames(x.reshape(x.shape[0], B, H, W, 3), kind).transpose(0, 1)
                util_vis.dump_gifs(opt, var.idx, name, frames, folder=folder)

    def dump_mesh_turntable(self, opt, var, folder):
        """{idx}_image_mesh_rotate.gif and {idx}_normal_mesh_rotate.gif of `--eval.mesh_render` in the vis_{ep}/ dump: the textured mesh from
        every pose of var.vis_pose at the size of the per-sample pictures, all views through ONE ops.mesh_raster call
        (eval_3D.mesh_render), frames by ops.vis_frames.  With `--mesh.ao` also {idx}_image_mesh_shaded_rotate.gif and
        {idx}_clay_mesh_rotate.gif: eval_3D.mesh_shade of those same views."""
        from .. import ops
        B = len(var.idx)
        H, W = (int(s) for s in var.mesh_render.render.depth.shape[-2:])
        pose = var.vis_pose[None].expand(B, -1, -1, -1)
        views = eval_3D.mesh_render(opt, var.level_vox, var.texture, pose, var.intr, H, W)
        frames = [("image_mesh_rotate", views.rgb), ("normal_mesh_rotate", views.normal)]
        if options.ao_settings(opt) is not None:
            frames += zip(("image_mesh_shaded_rotate", "clay_mesh_rotate"), eval_3D.mesh_shade(opt, var, views, pose))
        for name, x in frames:
            util_vis.dump_gifs(opt, var.idx, name, ops.vis_frames(x.contiguous(), "rgb"), folder=folder)

    def dump_geometry(self, opt, var, folder):
        """{idx}_mesh.ply (the predicted mesh) and {idx}_pointclouds_comp.ply (prediction red, ground truth green) of an evaluated batch;
        with --hip.mesh_color also {idx}_mesh_color.ply (the device mesh with vertex normals and the sample's predicted colours); with
        --eval.dual_mesh also {idx}_mesh_dual.ply (eval_3D.meshes_dual: the dual-contouring mesh of the same grid, positions and faces);
        with --eval.simplify also {idx}_mesh_simplified.ply (eval_3D.meshes_simplified: the mesh of {idx}_mesh.ply decimated by vertex
        clustering, positions and faces);
        with --mesh.smooth also {idx}_mesh_smooth.ply (eval_3D.meshes_smoothed: the mesh of {idx}_mesh.ply after Taubin smoothing, positions
        and the same faces) and {idx}_mesh_smooth.txt (one line: idx iters lambda mu vertices free fixed_boundary isolated degree_max
        disp_mean disp_max rough_before rough_after area_before area_after volume_before volume_after, lengths in object units);
        with --mesh.subdivide also {idx}_mesh_subdiv.ply (eval_3D.meshes_subdivided: the mesh of {idx}_mesh.ply after Loop subdivision and the
        Newton steps onto the SDF's zero set, positions and faces) and {idx}_mesh_subdiv.txt (one line: idx levels project vertices_in
        vertices_out faces_in faces_out edges sharp_edges fixed resid_before resid_after disp_mean disp_max area_before area_after
        volume_before volume_after, lengths in object units);
        with --mesh.decimate also {idx}_mesh_decimated.ply (eval_3D.meshes_decimated: the mesh of {idx}_mesh.ply brought to the face budget
        by quadric edge collapses, positions and faces) and {idx}_mesh_decimated.txt (one line: idx target vertices_in vertices_out
        faces_in faces_out rounds collapses rejected_link rejected_flip fixed reached dist_mean dist_max area_before area_after
        volume_before volume_after, lengths in object units);
        with --mesh.ao also {idx}_mesh_ao.ply (eval_3D.mesh_ambient_occlusion: the vertices and faces of {idx}_mesh.ply with the unit SDF
        normals and the ambient occlusion baked from the level grid as a grey in all three colour channels) and {idx}_mesh_ao.txt (one
        line: idx vertices radius step ao_mean ao_min ao_max open_share, radius and step in grid pitches); beside --eval.texture also
        {idx}_mesh_tex_ao.png (eval_3D.mesh_ao_atlas: the occlusion in the layout of the colour atlas; the OBJ and MTL keep their bytes)
        and beside --eval.mesh_render also {idx}_image_mesh_shaded.png and {idx}_clay_mesh.png (eval_3D.mesh_shade: the mesh picture and
        a plain grey one under the occlusion and a two-sided head light);
        with --mesh.self_intersect also {idx}_mesh_selfx.txt (eval_3D.mesh_intersections: one line per mesh variant written above, in the
        order mc dual simplified smooth subdiv decimated: idx variant faces degenerate box_pairs pairs pairs_vertex faces_hit first_face
        first_partner) and, for a variant with a face in a crossing pair only, {idx}_mesh_selfx_{variant}.ply (those faces alone);
        with --eval.icp also {idx}_pointclouds_comp_icp.ply (the ICP-aligned prediction of eval_3D.icp_metrics red, ground truth green);
        with --eval.normals also {idx}_pointclouds_normals.ply (pointclouds_comp's vertices as x y z nx ny nz red green blue: the SDF's
        normals on the prediction, the estimated PCA normals on the ground truth); with --eval.emd also {idx}_pointclouds_emd.ply (the
        two n-point sub-samples eval_3D.emd_metrics matched, prediction red, ground truth green); with --eval.iou also
        {idx}_voxels_comp.ply (the voxel centres of the two solids eval_3D.iou_metrics compared, likewise); with --eval.texture also
        {idx}_mesh_tex.obj / .mtl / .png and {idx}_mesh_tex_normal.png (eval_3D.mesh_texture: the device mesh with a per-triangle
        texture atlas of the predicted colours, and the atlas of its normals; var.texture keeps the result for texture.txt); with
        --eval.mesh_render also {idx}_image_mesh.png, {idx}_mask_mesh.png, {idx}_normal_mesh.png, {idx}_depth_mesh.png (the grey mapping
        of Renderer.surface_depth_grey) and {idx}_depth_mesh.npy: that textured mesh rasterised from the sample's own camera at the size
        of var.mask_input_map (eval_3D.mesh_render_sample; var.mesh_render keeps the result for mesh_render.txt; the texture is baked
        for it when --eval.texture is off, and no OBJ is written then).
        --eval.mesh_dist adds no per-sample file."""
        if eval_3D.HAVE_MESHING:
            meshes = var.mesh_pred                      # trimesh meshes of the PyMCubes branch
        else:
            lo, hi = opt.eval.range
            meshes = eval_3D.meshes_device(var.level_vox, lo, hi)
        util_vis.dump_meshes(opt, var.idx, "mesh", meshes, folder=folder)
        if _mesh_color(opt):
            net = self.graph.module
            coloured = eval_3D.mesh_attributes(opt, net.sdf_network, net.rgb_network, var.proj_latent_sdf, var.proj_latent_rgb, var.level_vox)
            util_vis.dump_meshes(opt, var.idx, "mesh_color", coloured, folder=folder)
        reg = options.dual_mesh_reg(opt)
        if reg is not None:
            net = self.graph.module
            # (--eval.mesh_dist measured against this mesh already and left it in var)
            dual = var.mesh_dual if "mesh_dual" in var else eval_3D.meshes_dual(opt, net.sdf_network, var.proj_latent_sdf, var.level_vox, reg)
            util_vis.dump_meshes(opt, var.idx, "mesh_dual", dual, folder=folder)
        if options.simplify_settings(opt) is not None:
            # (eval_metrics decimated the mesh already and left it in var)
            simple = var.mesh_simplified_world if "mesh_simplified_world" in var else eval_3D.meshes_simplified(opt, var)
            util_vis.dump_meshes(opt, var.idx, "mesh_simplified", simple, folder=folder)
        if options.smooth_settings(opt) is not None:
            # (eval_metrics smoothed the mesh already and left it in var)
            smooth = var.mesh_smoothed_world if "mesh_smoothed_world" in var else eval_3D.meshes_smoothed(opt, var)
            util_vis.dump_meshes(opt, var.idx, "mesh_smooth", smooth, folder=folder)
            util_vis.dump_lines(opt, var.idx, "mesh_smooth", eval_3D.smoothed_lines(var), folder=folder)
        if options.subdivide_settings(opt) is not None:
            # (eval_metrics refined the mesh already and left it in var)
            fine = (var.mesh_subdivided_world if "mesh_subdivided_world" in var
                    else eval_3D.meshes_subdivided(opt, var, self.graph.module.sdf_network))
            util_vis.dump_meshes(opt, var.idx, "mesh_subdiv", fine, folder=folder)
            util_vis.dump_lines(opt, var.idx, "mesh_subdiv", eval_3D.subdivided_lines(var), folder=folder)
        if options.decimate_settings(opt) is not None:
            # (eval_metrics decimated the mesh already and left it in var)
            few = var.mesh_decimated_world if "mesh_decimated_world" in var else eval_3D.meshes_decimated(opt, var)
            util_vis.dump_meshes(opt, var.idx, "mesh_decimated", few, folder=folder)
            util_vis.dump_lines(opt, var.idx, "mesh_decimated", eval_3D.decimated_lines(var), folder=folder)
        shade = options.ao_settings(opt) is not None
        if shade:
            # (eval_metrics baked the occlusion already and left it in var)
            lit = var.mesh_ao_world if "mesh_ao_world" in var else eval_3D.mesh_ambient_occlusion(opt, var, self.graph.module.sdf_network)
            util_vis.dump_meshes(opt, var.idx, "mesh_ao", lit, folder=folder)
            util_vis.dump_lines(opt, var.idx, "mesh_ao", eval_3D.ao_lines(var), folder=folder)
        if options.self_intersect_settings(opt):
            # (eval_metrics tested the meshes already and left the counts in var)
            if "mesh_intersections" not in var:
                eval_3D.mesh_intersections(opt, var, self.graph.module.sdf_network)
            util_vis.dump_lines(opt, var.idx, "mesh_selfx", eval_3D.intersection_lines(var), folder=folder)
            for variant in var.mesh_intersections:
                rows, hit = eval_3D.intersection_hit_meshes(opt, var, variant)
                util_vis.dump_meshes(opt, [var.idx[b] for b in rows], "mesh_selfx_" + variant, hit, folder=folder)
        if options.texture_texels(opt) is not None:
            net = self.graph.module
            var.texture = eval_3D.mesh_texture(opt, net.sdf_network, net.rgb_network, var.proj_latent_sdf, var.proj_latent_rgb, var.level_vox)
            util_vis.dump_textured_meshes(opt, var.idx, "mesh_tex", var.texture, folder=folder)
            if shade:
                util_vis.dump_atlases(opt, var.idx, "mesh_tex_ao", eval_3D.mesh_ao_atlas(opt, var, var.texture), folder=folder)
        if options.mesh_render(opt):
            net = self.graph.module
            if "texture" not in var:
                var.texture = eval_3D.mesh_texture(opt, net.sdf_network, net.rgb_network, var.proj_latent_sdf, var.proj_latent_rgb, var.level_vox)
            var.mesh_render = eval_3D.mesh_render_sample(opt, var, var.texture)
            out = var.mesh_render.render
            as_map = lambda x: x[:, 0].permute(0, 3, 1, 2) if x.dim() == 5 else x[:, 0, None]
            dump = lambda name, images: util_vis.dump_images(opt, var.idx, name, images, folder=folder)
            dump("image_mesh", as_map(out.rgb))
            dump("mask_mesh", as_map(out.mask))
            dump("normal_mesh", as_map(out.normal))
            dump("depth_mesh", as_map(eval_3D.mesh_depth_grey(opt, out, var.intr, var.scale_dist)))
            util_vis.dump_arrays(opt, var.idx, "depth_mesh", out.depth[:, 0], folder=folder)
            if shade:
                shaded, clay = eval_3D.mesh_shade(opt, var, out, var.pose)
                dump("image_mesh_shaded", as_map(shaded))
                dump("clay_mesh", as_map(clay))
        if "dpc" in var:
            util_vis.dump_pointclouds_compare(opt, var.idx, "pointclouds_comp", var.dpc_pred, var.dpc.points, folder=folder)
            if "dpc_pred_icp" in var:                   # --eval.icp: the ICP-aligned prediction red, the ground truth green
                util_vis.dump_pointclouds_compare(opt, var.idx, "pointclouds_comp_icp", var.dpc_pred_icp, var.dpc.points, folder=folder)
            if "normals_pred" in var:                   # --eval.normals: the clouds of pointclouds_comp with the normals that were compared
                util_vis.dump_pointclouds_compare(opt, var.idx, "pointclouds_normals", var.dpc_pred, var.dpc.points, folder=folder,
                                                  pred_normals=var.normals_pred, gt_normals=var.dpc.normals)
            if "emd" in var:                            # --eval.emd: what was matched
                sub_pred, sub_gt, _ = eval_3D.emd_subsample(var.dpc_pred, var.dpc.points, var.emd_n)
                util_vis.dump_pointclouds_compare(opt, var.idx, "pointclouds_emd", sub_pred, sub_gt, folder=folder)
            if "iou" in var:                            # --eval.iou: the voxel centres of the two solids that were compared
                centres = [[eval_3D.voxel_centres(bits[i], var.iou_origin[i], var.iou_pitch[i]) for i in range(len(var.idx))]
                           for bits in (var.iou_bits_pred, var.iou_bits_gt)]
                util_vis.dump_pointclouds_compare(opt, var.idx, "voxels_comp", centres[0], centres[1], folder=folder)

    @torch.no_grad()
    def dump_results(self, opt, var, ep, write_new=False, train=False):
        """The per-sample files of a batch (dump_visuals) and, outside training, its lines of chamfer.txt and of the per-sample files of
        every report of eval_reports.REPORTS that the batch carries."""
        self.dump_visuals(opt, var, ep, train=train)
        if not train:
            mode = "w" if write_new else "a"
            with open("{}/chamfer.txt".format(opt.output_path), mode) as f:
                for i, acc, comp in zip(var.idx, var.cd_acc, var.cd_comp):
                    f.write("{} {:.8f} {:.8f}\n".format(i, acc, comp))
            for rep in REPORTS:
                if rep.present(var, opt):
                    rep.write_lines(opt.output_path, rep.records(var), mode, opt)


    def save_checkpoint(self, opt, ep=0, it=0, best_val=np.inf, latest=False, best=False):
        assert _rank0(opt)
        util.save_checkpoint(opt, self, ep=ep, it=it, best_val=best_val, latest=latest, best=best)
        if not latest:
            log.info("checkpoint saved: ({0}) {1}, epoch {2} (iteration {3})".format(opt.group, opt.name, ep, it))
        if best:
            log.info("Saving the current model as the best...")
