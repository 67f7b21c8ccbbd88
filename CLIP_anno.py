"""python CLIP_anno.py --yaml=options/clip/pix3d.yaml [--data.pix3d.root=<tree>] [--clip_ckpt=<state dict>] [--hip.device_clip_preprocess!]
                      [--data.dataset=synthetic]

Offline CLIP nearest-neighbour annotation (reference CLIP_anno.py): embed every image of a split with
the CLIP image tower, L2-normalise, cosine k-NN, write `<anno_root>/<cat>_<split>.csv` with the header
Query,Top_1..Top_{k-1},Top_1_score..  sorted by query (same on-disk format; data/pix3d.py:95-108 reads it).

MI355X build: the tower runs on the HIP kernels (shapeclipper_amd/model/clip_vit.py; --clip_model=ViT-B/32
(default, BASELINE config[2]) or ViT-L/14 (the model the reference loads, CLIP_anno.py:16)); the O(N^2)
similarity is ONE GEMM + top-k instead of a Python loop (reference :29-57).  Weights: pass --clip_ckpt (a transformers CLIPVisionModelWithProjection or
openai/CLIP state dict); without it the tower is randomly initialised (no network here).

Pix3D (reference :129-182): the splits val, train, test of data/pix3d.py in its CLIP-annotation mode, in loader order, labelled by
the dataset's rel_path_list; per split CLIP_NN_{split}.png (save_vis) in opt.output_path and the CSV.  The tower's input is the
reference's composite + CLIP preprocess (data/clip_preprocess.py): by default computed for each batch on the device from the
workers' uint8 RGBA images (csrc/clip_preprocess.hip), with --hip.device_clip_preprocess! in the workers on the CPU; both give the
same bits."""
import csv
import importlib
import os
import sys

import torch
import torch.nn.functional as torch_F

import utils.options as options
from utils.util import log
from shapeclipper_amd.model.clip_vit import VIT_B32, VIT_L14, ClipVisionTower


class NN_annotator:
    def __init__(self, opt):
        name = str(opt.get("clip_model", "ViT-B/32"))
        if name not in ("ViT-B/32", "ViT-L/14"):
            raise NotImplementedError("clip_model '%s' (available: ViT-B/32, ViT-L/14)" % name)
        cfg = VIT_L14 if name == "ViT-L/14" else VIT_B32
        cfg = dict(cfg, dtype=str(opt.get("clip_dtype", "fp16")))       # fp16: the reference's arithmetic on a GPU (:16); or bf16
        self.tower = ClipVisionTower(**cfg)
        ckpt = opt.get("clip_ckpt", None)
        if ckpt:
            sd = torch.load(ckpt, map_location="cpu")
            if any(k.startswith("visual.") for k in sd):
                self.tower = ClipVisionTower.from_openai_state_dict(sd, **cfg)
            else:
                self.tower.load_state_dict(sd)
        self.tower = self.tower.to(opt.device)
        self.clip_dim = cfg["proj"]
        self.n_px = cfg["image_size"]

    @torch.no_grad()
    def calc_matches(self, opt, features, k_nearest=6):
        """features [N,D] L2-normalised -> (indices [N,k], values [N,k]); row i starts with i itself
        (reference CLIP_anno.py:29-57).

        Default (opt.thres is None): ONE similarity GEMM + top-k instead of the reference's per-query Python loop.
        Thresholded branch (:43-53, off in options/clip/pix3d.yaml): k-1 random neighbours among cos >= thres; it keeps
        the reference's per-query operator sequence -- (query * features).sum(1), the `< 1.` test that is meant to drop
        the query itself (a query whose self-similarity rounds to 0.99999994 stays a candidate, as in the reference) and
        one CPU-generator randperm per qualifying query, in query order -- so a seeded run picks the same neighbours."""
        if opt.thres is None:
            values, indices = (features @ features.t()).topk(k_nearest, dim=1, largest=True)
            return indices, values
        indices, values = [], []
        for i in range(features.shape[0]):
            cos_sim = (features[i].unsqueeze(0) * features).sum(dim=1)
            index = ((cos_sim >= opt.thres) & (cos_sim < 1.)).nonzero()
            n_valid = len(index)
            if n_valid < k_nearest - 1:
                top_k_val, top_k_ind = cos_sim.topk(k_nearest, largest=True)
                indices.append(top_k_ind)
                values.append(top_k_val)
            else:
                sampled = index[torch.randperm(n_valid)[:k_nearest - 1].to(index.device)].squeeze(1)
                chosen = torch.cat([torch.tensor([i], device=features.device), sampled], dim=0)
                indices.append(chosen)
                values.append(cos_sim[chosen])
        return torch.stack(indices, dim=0), torch.stack(values, dim=0)

    def label2path(self, root, label):
        return os.path.join(root, label), None

    def save_vis(self, opt, label2path, root, labels, ind, values, k_nearest=6, n_vis=15):
        """CLIP_NN_{split}.png in opt.output_path: n_vis rows (queries N // n_vis * i), each the query and its k_nearest - 1
        neighbours with their similarity (reference CLIP_anno.py:59-96)."""
        import matplotlib
        matplotlib.use("Agg")
        import matplotlib.pyplot as plt
        from PIL import Image
        N = len(labels)
        count = 1
        fig = plt.figure(figsize=(5 * k_nearest, 5 * n_vis))
        for i in [N // n_vis * v for v in range(n_vis)]:
            plt.subplot(n_vis, k_nearest, count)
            plt.imshow(Image.open(label2path(root, labels[i])[0]).convert("RGB"))
            plt.xticks([])
            plt.yticks([])
            count += 1
            for j, index in enumerate(ind[i][1:]):
                plt.subplot(n_vis, k_nearest, count)
                plt.imshow(Image.open(label2path(root, labels[int(index)])[0]).convert("RGB"))
                plt.title("{:.3f}".format(values[i, j + 1].item()), fontweight="bold")
                plt.xticks([])
                plt.yticks([])
                count += 1
        plt.tight_layout()
        path = os.path.join(opt.output_path, "CLIP_NN_{}.png".format(self.split))
        plt.savefig(path)
        plt.close(fig)
        return path

    def save_anno(self, opt, label2path, labels, index_topk, value_topk, k_nearest=6, category_set="all"):
        """`<anno_root>/<category>_<split>.csv`, header Query,Top_1..,Top_1_score.., rows sorted by query
        (reference CLIP_anno.py:98-127; read back by data/pix3d.py:95-108).  self.split names the split."""
        category = opt.data[opt.data.dataset].cat.replace(", ", "_") if category_set == "custom" else category_set
        os.makedirs(opt.anno_root, exist_ok=True)
        path = os.path.join(opt.anno_root, "{}_{}.csv".format(category, self.split))
        rows = []
        for i, label in enumerate(labels):
            rows.append([label2path("", label)[0]] + [label2path("", labels[int(j)])[0] for j in index_topk[i][1:]]
                        + ["{:.4f}".format(v) for v in value_topk[i][1:]])
        header = ["Query"] + ["Top_{}".format(i) for i in range(1, k_nearest)] + ["Top_{}_score".format(i) for i in range(1, k_nearest)]
        with open(path, "w") as f:
            w = csv.writer(f)
            w.writerow(header)
            w.writerows(sorted(rows, key=lambda r: r[0]))
        return path

    @torch.no_grad()
    def embed_split(self, opt, images):
        return self.embed_batches(opt, (images[i:i + opt.batch_size] for i in range(0, len(images), opt.batch_size)))

    @torch.no_grad()
    def embed_batches(self, opt, batches):
        """L2-normalised embeddings [N,D] of an iterable of image batches [b,3,n_px,n_px]."""
        feats = []
        for images in batches:
            e = self.tower.encode_image(images.to(opt.device)).float()
            feats.append(torch_F.normalize(e, dim=-1))
        feats = torch.cat(feats, dim=0)
        # the small-batch tower reports a cluster-barrier time-out (its members were not co-resident: another kernel held CUs) by poisoning
        # the class-token row, i.e. as NaN embeddings (csrc/clip_cluster.hpp); a nearest-neighbour table must never be built from those
        if not bool(torch.isfinite(feats).all()):
            bad = (~torch.isfinite(feats).all(dim=1)).nonzero().flatten().tolist()
            raise RuntimeError("CLIP tower produced non-finite embeddings for %d image(s) (first: %s): a cluster-barrier time-out of the small-batch "
                               "kernel or non-finite inputs; re-run with SC_CLIP_CLUSTER_MAX_B=0 to take the launch-per-operation form" % (len(bad), bad[:5]))
        return feats


def pix3d_splits(opt, ann):
    """{split: (embeddings [N,D], labels)} for val, train, test of data/pix3d.py in the CLIP-annotation mode (reference :140-166)."""
    from shapeclipper_amd.data.clip_preprocess import ClipPreprocess
    from shapeclipper_amd.data.pix3d import device_clip_preprocess
    data = importlib.import_module("data.{}".format(opt.data.dataset))
    pre = ClipPreprocess(ann.n_px, opt.data.bgcolor)
    on_device = device_clip_preprocess(opt)
    pin = str(opt.device).startswith("cuda")
    out = {}
    for split in ("val", "train", "test"):
        log.info("loading {} data...".format(split))
        ds = data.Dataset(opt, split=split, transform=pre)
        loader = torch.utils.data.DataLoader(ds, batch_size=opt.batch_size, num_workers=opt.data.num_workers, shuffle=False,
                                             drop_last=False, pin_memory=pin)
        if on_device:
            batches = (pre.device(b["rgba_input"].to(opt.device, non_blocking=True)) for b in loader)
        else:
            batches = (b["rgb_input"].to(opt.device, non_blocking=True) for b in loader)
        out[split] = (ann.embed_batches(opt, batches), list(ds.rel_path_list), os.path.join(ds.path, "img_processed"))
    return out


def main():
    log.process(os.getpid())
    log.title("[{}] (compute CLIP-NN)".format(sys.argv[0]))
    opt = options.set(opt_cmd=options.parse_arguments(sys.argv[1:]))
    ann = NN_annotator(opt)
    if opt.data.dataset.startswith("pix3d"):
        for split, (feats, labels, root_image) in pix3d_splits(opt, ann).items():
            idx, val = ann.calc_matches(opt, feats, k_nearest=opt.k_nearest)
            ann.split = split
            idx, val = idx.cpu(), val.cpu()
            print("wrote", ann.save_vis(opt, ann.label2path, root_image, labels, idx, val, k_nearest=opt.k_nearest, n_vis=15))
            print("wrote", ann.save_anno(opt, ann.label2path, labels, idx, val, k_nearest=opt.k_nearest, category_set="custom"))
        return
    if opt.data.dataset == "synthetic":
        n = int(opt.data.get("synthetic_len", 256))
        gen = torch.Generator().manual_seed(0)
        images = torch.randn(n, 3, 224, 224, generator=gen)
        labels = ["synthetic/img_{:05d}.png".format(i) for i in range(n)]
        splits = {"train": (images, labels)}
    else:
        raise NotImplementedError("data.dataset '%s' (available: pix3d, synthetic)" % opt.data.dataset)
    for split, (images, labels) in splits.items():
        feats = ann.embed_split(opt, images)
        idx, val = ann.calc_matches(opt, feats, k_nearest=opt.k_nearest)
        ann.split = split
        custom = "custom" if opt.data.dataset in opt.data else "all"
        print("wrote", ann.save_anno(opt, ann.label2path, labels, idx.cpu(), val.cpu(), k_nearest=opt.k_nearest, category_set=custom))


if __name__ == "__main__":
    main()
