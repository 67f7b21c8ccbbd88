"""Pix3D loader with the reference's semantics (data/pix3d.py, data/base.py), quirks included; line numbers refer to the reference's
data/pix3d.py.  torchvision is not used: PIL + numpy restate `to_tensor` exactly (uint8 HWC -> float32 CHW / 255).

Expected tree under `root` (the reference hard-codes data/Pix3D; `--data.pix3d.root` overrides it), as in the reference's processed
download:
    lists/{cat}_{split}.txt                  one sample name per line
    annotation/{cat}/{name}.json             Pix3D's annotation: img, mask, model, focal_length, cam_position, rot_mat, trans_mat, bbox
    img_processed/..., mask_processed/..., normal_processed/...   (the annotation's img / mask paths with the words replaced)
    pointclouds/{model path without "model/", .npy}
    CLIP_NN/{cat}_{split}.csv                query path, then its neighbours (CLIP_anno.py's output)

CLIP-annotation mode (`transform=ClipPreprocess(n_px, bgcolor)`, CLIP_anno.py): no CLIP_NN read; `rel_path_list`, `img_path_list` and
`pc_path_list` are built instead, and a sample is {idx, rgba_input}: the RGBA image resized to (W, H) as uint8 [H, W, 4], which
ClipPreprocess.device turns into the tower's input for a whole batch (csrc/clip_preprocess.hip).  With
`--hip.device_clip_preprocess!` the sample is the reference's {idx, rgb_input}, the fp32 input computed in the worker.

Rays (train split, render.rand_sample): with `hip.device_rays` (default) the workers draw no rays; every sample carries
`ray_seed [1+K] int64` and `sample_rays_device` draws all B x (1+K) views of a batch on the device (csrc/silhouette_rays.hip).  With
`--hip.device_rays!` each view's rays come from utils.util.compute_sampling_prob in the worker, the reference's procedure
(:230-239) and numpy stream."""
import csv
import json
from copy import deepcopy

import numpy as np
import PIL.Image
import torch
import torch.nn.functional as torch_F

from ..utils import camera, options, util
from ..utils.util import EasyDict as edict
from .clip_preprocess import ClipPreprocess

DEFAULT_ROOT = "data/Pix3D"
_GOLDEN = 0x9E3779B97F4A7C15


def to_tensor(image):
    """torchvision.transforms.functional.to_tensor for 8-bit PIL images: [C,H,W] float32 = uint8 / 255."""
    arr = np.array(image, dtype=np.uint8)
    if arr.ndim == 2:
        arr = arr[:, :, None]
    return torch.from_numpy(arr).permute(2, 0, 1).contiguous().float().div(255)


def device_rays(opt):
    return bool(options.hip(opt, "device_rays"))


def device_clip_preprocess(opt):
    return bool(options.hip(opt, "device_clip_preprocess"))


def ray_seeds(base, idx, n_views):
    """ray_seed [n_views] int64: the worker's numpy draw `base` mixed with the sample index and the view number (Weyl step of
    splitmix64), so that two samples -- on one rank or on two -- never share a seed even when their workers' numpy streams agree."""
    out = [(int(base) + (int(idx) * n_views + v + 1) * _GOLDEN) % (1 << 64) for v in range(n_views)]
    return torch.tensor(np.array(out, dtype=np.uint64).view(np.int64))


class Dataset(torch.utils.data.Dataset):

    def __init__(self, opt, split="train", transform=None):
        super().__init__()
        self.opt = deepcopy(opt)               # base.Dataset: later changes of opt.H / opt.W (evaluate) do not reach the maps
        self.split = split
        self.augment = split == "train" and opt.data.augment
        self.cat_id_all = dict(bed="bed", bookcase="bookcase", chair="chair", desk="desk", misc="misc", sofa="sofa", table="table",
                               tool="tool", wardrobe="wardrobe")                                            # :15-27
        # :29-31: a transform puts the dataset in the CLIP-annotation mode (CLIP_anno.py); the transform is the reference's composite
        # plus CLIP's preprocess, restated as ClipPreprocess
        if transform is not None and not isinstance(transform, ClipPreprocess):
            raise NotImplementedError("data.pix3d: the CLIP-annotation mode takes a data.clip_preprocess.ClipPreprocess transform "
                                      "(CLIP_anno.py), got %r" % (transform,))
        self.clip_anno = transform is not None
        self.transform = transform
        self.max_imgs = opt.data.max_img_cat if opt.data.max_img_cat is not None else np.inf
        self.cat2label = {}
        accum_idx = 0
        self.cat_id = list(self.cat_id_all.values()) if opt.data.pix3d.cat is None else \
            [v for k, v in self.cat_id_all.items() if k in opt.data.pix3d.cat.split(",")]                # :35-36
        for cat in self.cat_id:
            self.cat2label[cat] = accum_idx
            accum_idx += 1
        self.label2cat = []
        for cat in self.cat_id:
            key = next(key for key, value in self.cat_id_all.items() if value == cat)
            self.label2cat.append(key)
        self.path = opt.data.pix3d.get("root", None) or DEFAULT_ROOT                                        # :45
        self.list = self.get_list(opt, split)
        if self.clip_anno:
            self.get_path_list(opt)                                                                         # :46-49
        else:
            self.NN_dict = self.get_NN_anno(opt)

    # :51-60 -- [(category, sample name)], at most max_img_cat per category
    def get_list(self, opt, split):
        cads = []
        for c in self.cat_id:
            list_fname = "{}/lists/{}_{}.txt".format(self.path, c, split)
            with open(list_fname) as f:
                lines = f.read().splitlines()
            for i, m in enumerate(lines):
                if i >= self.max_imgs:
                    break
                cads.append((c, m))
        return cads

    def get_path_list(self, opt):                                                                          # :62-72
        self.img_path_list, self.pc_path_list, self.rel_path_list = [], [], []
        for idx in range(len(self.list)):
            meta = self.get_metadata(opt, idx)
            self.pc_path_list.append("{0}/{1}".format(self.path, "pointclouds/" + meta.cad_path[6:]).replace(".obj", ".npy"))
            self.img_path_list.append("{0}/{1}".format(self.path, meta.img_path))
            self.rel_path_list.append("/".join(meta.img_path.split("/")[1:]))

    def name_from_path(self, opt, relpath):                                                                # :74-77
        c = relpath.split("/")[0]
        name = relpath.split("/")[1].split(".")[0]
        return c, name

    def id_filename_mapping(self, opt, outpath):                                                           # :79-91
        with open(outpath, "w") as outfile:
            for i in range(len(self.list)):
                meta = self.get_metadata(opt, i)
                image_fname = "{0}/{1}".format(self.path, meta.img_path)
                mask_fname = "{0}/{1}".format(self.path, meta.mask_path)
                normal_path = meta.mask_path.replace("mask", "normal")
                normal_fname = "{0}/{1}".format(self.path, normal_path)
                pc_fname = "{0}/{1}".format(self.path, "pointclouds/" + meta.cad_path[6:])
                pc_fname = pc_fname.replace(".obj", ".npy")
                outfile.write("{} {} {} {} {}\n".format(i, image_fname, mask_fname, normal_fname, pc_fname))

    # :95-108 -- {(c, name): [(c_n, name_n)] * k_nearest}
    def get_NN_anno(self, opt):
        dict_anno = {}
        category_name = opt.data[opt.data.dataset].cat.replace(", ", "_")
        NN_fname = "{}/CLIP_NN/{}_{}.csv".format(self.path, category_name, self.split)
        with open(NN_fname, "r") as csvfile:
            list_anno = list(csv.reader(csvfile))[1:]
        for anno in list_anno:
            c, name = self.name_from_path(opt, anno[0])
            dict_anno[(c, name)] = []
            for nearest in anno[1:1 + opt.data.k_nearest]:
                dict_anno[(c, name)].append(self.name_from_path(opt, nearest))
        return dict_anno

    def __getitem__(self, idx):                                                                            # :110-228
        opt = self.opt
        sample = dict(idx=idx)
        meta = self.get_metadata(opt, idx)
        if self.clip_anno:                                                                                  # :117-121
            image = self.get_image(opt, meta=meta).resize((opt.W, opt.H))
            if device_clip_preprocess(opt):
                sample.update(rgba_input=torch.from_numpy(np.array(image, dtype=np.uint8)))      # ClipPreprocess.device on the batch
            else:
                sample.update(rgb_input=self.transform(image))
            return sample
        image = self.get_image(opt, meta=meta)
        cat_label, _ = self.get_category(opt, idx)
        rgb_input_map, mask_input_map = self.preprocess_image(opt, image)
        normal_input_map = self.get_normal(opt, meta, mask_input_map)
        sample.update(rgb_input_map=rgb_input_map, mask_input_map=mask_input_map, normal_input_map=normal_input_map,
                      category_label=cat_label)
        rgb_input, mask_input, normal_input, ray_idx = self.sample_map(opt, rgb_input_map, mask_input_map, normal_input_map)
        if rgb_input is not None:
            sample.update(rgb_input=rgb_input, mask_input=mask_input, normal_input=normal_input)
        if ray_idx is not None:
            sample.update(ray_idx=ray_idx)
        intr, pose = self.get_camera(opt, meta=meta)
        sample.update(pose_gt=pose, intr=intr)
        sample.update(dpc=self.get_pointcloud(opt, idx, meta=meta))
        c, name = self.list[idx]
        neighbors = self.NN_dict[(c, name)]
        maps = dict(rgb=[], mask=[], normal=[])
        flat = dict(rgb=[], mask=[], normal=[])
        ray_idx_NN_list, pose_NN_list = [], []
        for i in range(opt.data.k_nearest):
            c_n, name_n = neighbors[i]
            meta_n = self.get_metadata(opt, 0, name_n, c_n)
            input_NN = self.get_NN(opt, meta_n, c_n)
            maps["rgb"].append(input_NN.rgb_input_map)
            maps["mask"].append(input_NN.mask_input_map)
            maps["normal"].append(input_NN.normal_input_map)
            rgb_n, mask_n, normal_n, ray_idx_n = self.sample_map(opt, input_NN.rgb_input_map, input_NN.mask_input_map,
                                                                 input_NN.normal_input_map)
            pose_NN = self.get_camera(opt, meta=meta)[1]           # :192: the QUERY's metadata (a reference quirk, kept)
            if ray_idx_n is not None:
                ray_idx_NN_list.append(ray_idx_n)
            flat["rgb"].append(rgb_n)
            flat["mask"].append(mask_n)
            flat["normal"].append(normal_n)
            pose_NN_list.append(pose_NN)
        for k in ("rgb", "mask", "normal"):
            if flat[k][0] is not None:
                sample["{}_input_NN".format(k)] = torch.stack(flat[k], dim=-1)
            sample["{}_input_map_NN".format(k)] = torch.stack(maps[k], dim=-1)
        sample.update(pose_gt_NN=torch.stack(pose_NN_list, dim=-1))
        if len(ray_idx_NN_list) > 0:
            sample.update(ray_idx_NN=torch.stack(ray_idx_NN_list, dim=-1))
        if self._rays_on_device(opt):
            sample.update(ray_seed=ray_seeds(np.random.randint(0, 2 ** 63, dtype=np.int64), idx, 1 + opt.data.k_nearest))
        return sample

    def _rays_on_device(self, opt):
        return self.split == "train" and bool(opt.render.rand_sample) and device_rays(opt)

    # :230-240 -- the train split samples rand_sample rays per view; the test split keeps all H*W pixels
    def sample_map(self, opt, rgb_map, mask_map, normal_map):
        if self._rays_on_device(opt):
            return None, None, None, None            # sample_rays_device draws the rays and fills the sampled inputs
        rgb = rgb_map.permute(1, 2, 0).view(opt.H * opt.W, 3)
        mask = mask_map.permute(1, 2, 0).view(opt.H * opt.W, 1)
        normal = normal_map.permute(1, 2, 0).view(opt.H * opt.W, 3)
        ray_idx = None
        if self.split == "train" and opt.render.rand_sample:
            ray_idx = util.compute_sampling_prob(opt, mask_map[0], opt.render.ray_uniform_fac)
            rgb, mask = rgb[ray_idx], mask[ray_idx]
            normal = normal[ray_idx]
        return rgb, mask, normal, ray_idx

    def get_NN(self, opt, meta, category):                                                                 # :242-251
        image = self.get_image(opt, meta=meta)
        rgb, mask = self.preprocess_image(opt, image)
        normal = self.get_normal(opt, meta, mask)
        return edict(rgb_input_map=rgb, mask_input_map=mask, normal_input_map=normal)

    def get_image(self, opt, meta):                                                                        # :253-259
        image = PIL.Image.open("{0}/{1}".format(self.path, meta.img_path)).convert("RGB")
        mask = PIL.Image.open("{0}/{1}".format(self.path, meta.mask_path)).convert("L")
        return PIL.Image.merge("RGBA", (*image.split(), mask))

    def get_normal(self, opt, meta, mask):                                                                 # :261-271
        normal_path = meta.mask_path.replace("mask", "normal")
        normal = PIL.Image.open("{0}/{1}".format(self.path, normal_path)).convert("RGB")
        normal = normal.resize((opt.W, opt.H))
        normal = to_tensor(normal)
        assert normal.shape[0] == 3
        normal = (normal - 0.5) * 2
        normal = torch_F.normalize(normal, dim=0, p=2)
        return normal * mask

    def get_category(self, opt, idx):                                                                      # :273-276
        c, _ = self.list[idx]
        return int(self.cat2label[c]), c

    def preprocess_image(self, opt, image):                                                                # :278-289
        # RGBA resized as ONE image: Pillow resizes RGBA premultiplied, so the RGB values near the silhouette differ from a
        # channel-by-channel resize
        image = image.resize((opt.W, opt.H))
        image = to_tensor(image)
        rgb, mask = image[:3], image[3:]
        mask = (mask > 0.5).float()
        if opt.data.bgcolor is not None:
            rgb = rgb * mask + opt.data.bgcolor * (1 - mask)
        return rgb, mask

    def get_camera(self, opt, meta=None):                                                                  # :291-305
        intr = torch.tensor([[opt.camera.focal * opt.W, 0, opt.W / 2],
                             [0, opt.camera.focal * opt.H, opt.H / 2],
                             [0, 0, 1]])
        R_raw = meta.cam.R
        R_trans = torch.tensor([[1, 0, 0], [0, 1, 0], [0, 0, -1]]).float().to(R_raw.device)
        R = torch.mm(R_trans, R_raw)
        pose_R = camera.pose(R=R)
        pose_T = camera.pose(t=[0, 0, opt.camera.dist])
        return intr, camera.pose.compose([pose_R, pose_T])

    def get_pointcloud(self, opt, idx, meta=None):                                                         # :307-315
        pc_fname = "{0}/{1}".format(self.path, "pointclouds/" + meta.cad_path[6:]).replace(".obj", ".npy")
        pc = torch.from_numpy(np.load(pc_fname)).float()
        return dict(points=pc, normals=torch.zeros_like(pc))

    def get_metadata(self, opt, idx, name=None, c=None):                                                   # :328-348
        if name is None or c is None:
            c, name = self.list[idx]
        with open("{}/annotation/{}/{}.json".format(self.path, c, name), "r", encoding="utf-8") as f:
            meta = json.load(f)
        return edict(
            cam=edict(focal=float(meta["focal_length"]), cam_loc=torch.tensor(meta["cam_position"]), R=torch.tensor(meta["rot_mat"]),
                      T=torch.tensor(meta["trans_mat"])),
            img_path=meta["img"].replace("img", "img_processed"),           # str.replace: every occurrence
            mask_path=meta["mask"].replace("mask", "mask_processed"),
            cad_path=meta["model"],
            bbox=torch.tensor(meta["bbox"]),
        )

    def __len__(self):
        return len(self.list)

    def setup_loader(self, opt, shuffle=False, drop_last=True, subcat=None, batch_size=None, allow_ddp=True):        # base.py:16-30
        sampler = None
        if self.split == "train" and allow_ddp and "world_size" in opt:
            sampler = torch.utils.data.distributed.DistributedSampler(self, num_replicas=opt.world_size, rank=util.get_rank(opt))
        loader = torch.utils.data.DataLoader(self, batch_size=batch_size if batch_size is not None else opt.batch_size,
                                             num_workers=opt.data.num_workers, shuffle=shuffle if sampler is None else False,
                                             drop_last=drop_last, sampler=sampler)
        if util.get_rank(opt) == 0:
            print("number of samples: {}".format(len(self)))
        return loader


def sample_rays_device(opt, var):
    """Draw the rays of a training batch on the device: silhouette distance and weighted draw over all B x (1+K) masks in two
    launches (ops.silhouette_distance / ops.silhouette_rays), then fill ray_idx [B,R], ray_idx_NN [B,R,K] and the sampled
    rgb / mask / normal inputs and their _NN stacks, as the loader's compute_sampling_prob branch lays them out.  Batches without
    `ray_seed` (synthetic data, the test split, --hip.device_rays!) are returned unchanged."""
    if "ray_seed" not in var:
        return var
    from .. import ops
    mask_map, mask_map_NN = var.mask_input_map, var.mask_input_map_NN           # [B,1,H,W], [B,1,H,W,K]
    B, _, H, W = mask_map.shape
    K = mask_map_NN.shape[-1]
    R = int(opt.render.rand_sample)
    masks = torch.cat([mask_map, mask_map_NN[:, 0].permute(0, 3, 1, 2)], dim=1).reshape(B * (1 + K), H, W)
    dist = ops.silhouette_distance(masks)
    ray_idx = ops.silhouette_rays(dist, R, float(opt.render.ray_uniform_fac), var.ray_seed.reshape(-1).contiguous()).view(B, 1 + K, R)
    var.ray_idx = ray_idx[:, 0].contiguous()
    var.ray_idx_NN = ray_idx[:, 1:].permute(0, 2, 1).contiguous()

    def take(m, idx):             # [B,C,H,W], [B,R] -> [B,R,C]
        C = m.shape[1]
        return m.reshape(B, C, H * W).gather(2, idx[:, None, :].expand(B, C, R)).permute(0, 2, 1).contiguous()

    for key in ("rgb", "mask", "normal"):
        m, m_NN = var[key + "_input_map"], var[key + "_input_map_NN"]
        var[key + "_input"] = take(m, var.ray_idx)
        var[key + "_input_NN"] = torch.stack([take(m_NN[..., k], var.ray_idx_NN[..., k]) for k in range(K)], dim=-1)
    return var
