"""Writes tests/golden/video_transforms.npz: what the reference's own ``datasets/video_transforms.py`` computes (torch, CPU) for the
three frame pipelines of ``datasets/__init__.py:13-76`` on small random uint8 clips, its temporal windows, and the intermediate
sizes / crop offsets / crop errors of ``UCFCenterCropVideo`` and ``CenterCropResizeVideo`` at a few source sizes.

The reference file is loaded BY PATH and run as it is.  torchvision is not needed: ``torchvision.transforms`` is a stand-in module
holding the two names the file imports (``RandomCrop``, ``RandomResizedCrop``, unused by the pipelines), and the pipelines are
composed with ``Compose`` / ``Normalize`` below, which restate torchvision's (call in order; ``tensor.sub_(mean).div_(std)``).

  python tools/make_video_transform_golden.py --reference /path/to/Latte
"""
import argparse
import importlib.util
import json
import os
import random
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load_reference(root):
    tv, tvt = types.ModuleType("torchvision"), types.ModuleType("torchvision.transforms")
    tvt.RandomCrop = tvt.RandomResizedCrop = None
    tv.transforms = tvt
    sys.modules.setdefault("torchvision", tv)
    sys.modules.setdefault("torchvision.transforms", tvt)
    spec = importlib.util.spec_from_file_location("ref_video_transforms", os.path.join(root, "datasets", "video_transforms.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


class Compose:
    def __init__(self, ts):
        self.ts = ts

    def __call__(self, x):
        for t in self.ts:
            x = t(x)
        return x


class Normalize:
    def __init__(self, mean, std, inplace=False):
        self.mean, self.std, self.inplace = mean, std, inplace

    def __call__(self, x):
        x = x if self.inplace else x.clone()
        mean = torch.as_tensor(self.mean, dtype=x.dtype).view(-1, 1, 1)
        std = torch.as_tensor(self.std, dtype=x.dtype).view(-1, 1, 1)
        return x.sub_(mean).div_(std)


def pipeline(vt, dataset, size, p_flip):
    """The Compose of datasets/__init__.py for `dataset`, with the flip probability pinned to 0 or 1."""
    norm = Normalize(mean=[0.5, 0.5, 0.5], std=[0.5, 0.5, 0.5], inplace=True)
    if dataset in ("ffs", "ucf101"):
        return Compose([vt.ToTensorVideo(), vt.RandomHorizontalFlipVideo(p_flip), vt.UCFCenterCropVideo(size), norm])
    if dataset == "taichi":
        return Compose([vt.ToTensorVideo(), vt.RandomHorizontalFlipVideo(p_flip), norm])
    if dataset == "sky":
        return Compose([vt.ToTensorVideo(), vt.CenterCropResizeVideo(size), norm])
    raise NotImplementedError(dataset)


def geometry(vt, kind, hs, ws, size):
    """(mid_h, mid_w, crop_i, crop_j, reg_y, reg_x) as the reference's functions produce them, read off coordinate-valued clips."""
    yy = torch.arange(hs, dtype=torch.float32).view(1, 1, hs, 1).expand(1, 1, hs, ws)
    xx = torch.arange(ws, dtype=torch.float32).view(1, 1, 1, ws).expand(1, 1, hs, ws)
    if kind == "ucf":
        mid = vt.resize_scale(torch.zeros(1, 1, hs, ws), (size, size), "bilinear")
        mh, mw = mid.shape[-2:]
        my = torch.arange(mh, dtype=torch.float32).view(1, 1, mh, 1).expand(1, 1, mh, mw)
        mx = torch.arange(mw, dtype=torch.float32).view(1, 1, 1, mw).expand(1, 1, mh, mw)
        ci = int(vt.center_crop(my, (size, size))[0, 0, 0, 0])
        cj = int(vt.center_crop(mx, (size, size))[0, 0, 0, 0])
        return [mh, mw, ci, cj, 0, 0]
    ry = int(vt.center_crop_using_short_edge(yy)[0, 0, 0, 0])
    rx = int(vt.center_crop_using_short_edge(xx)[0, 0, 0, 0])
    return [size, size, 0, 0, ry, rx]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of the reference repository (its datasets/video_transforms.py is run)")
    a = ap.parse_args()
    vt = load_reference(a.reference)
    out = {}
    # ---- temporal windows: totals below, equal to and above size + 1, from random.seed(SEED)
    size, num_frames, seed = 8, 4, 11
    totals = [3, 7, 8, 9, 10, 20, 57, 200]
    random.seed(seed)
    crop = vt.TemporalRandomCrop(size)
    windows = []
    for total in totals:
        for _ in range(4):
            windows.append([total, *crop(total)])
    windows = np.array(windows, dtype=np.int64)
    out["temporal_windows"] = windows
    out["temporal_indices"] = np.stack([np.linspace(b, e - 1, num_frames, dtype=int) for _, b, e in windows]).astype(np.int64)
    out["temporal_params"] = np.array([size, num_frames, seed], dtype=np.int64)
    # ---- geometry at the sizes the planner is checked at (no pixels kept)
    geo = [("ucf", 240, 320, 256), ("ucf", 321, 240, 256), ("ucf", 37, 53, 16), ("ucf", 300, 200, 128), ("ucf", 5, 7, 8),
           ("sky", 180, 320, 128), ("sky", 45, 28, 24), ("sky", 31, 36, 16)]
    out["geometry_cases"] = np.frombuffer(json.dumps(geo).encode(), dtype=np.uint8)
    out["geometry"] = np.array([geometry(vt, *g) for g in geo], dtype=np.int64)
    # ---- which short edges make UCFCenterCropVideo(256) raise: floor(short * (256 / short)) < 256 in double
    raising = []
    for short in range(1, 400):
        try:
            vt.UCFCenterCropVideo(256)(torch.zeros(1, 1, short, short + 3))
        except ValueError as e:
            assert str(e) == "height and width must be no smaller than crop_size", e
            raising.append(short)
    out["ucf256_raising_short_edges"] = np.array(raising, dtype=np.int64)
    # ---- pixels: dataset, frames, Hs, Ws, size (0 = keep)
    g = torch.Generator().manual_seed(3)
    cases = [("ucf101", 2, 37, 48, 16), ("ffs", 1, 20, 13, 16), ("sky", 1, 30, 47, 16), ("sky", 1, 45, 28, 24), ("taichi", 1, 24, 18, 0)]
    out["pixel_cases"] = np.frombuffer(json.dumps(cases).encode(), dtype=np.uint8)
    for k, (dataset, n, hs, ws, s) in enumerate(cases):
        x = torch.randint(0, 256, (n, hs, ws, 3), generator=g, dtype=torch.uint8)
        out[f"pixel{k}_in"] = x.numpy()
        tchw = x.permute(0, 3, 1, 2)
        out[f"pixel{k}_out"] = pipeline(vt, dataset, s, 0.0)(tchw).contiguous().numpy()
        if dataset != "sky":
            out[f"pixel{k}_out_flipped"] = pipeline(vt, dataset, s, 1.0)(tchw).contiguous().numpy()
    path = os.path.join(ROOT, "tests", "golden", "video_transforms.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes; raising short edges below 400:", raising)


if __name__ == "__main__":
    main()
