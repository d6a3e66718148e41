#!/usr/bin/env python3
"""FID and improved precision / recall between two folders of images, on CLIP ViT-B/32 image features (rdm_amd.metrics): what the
reference's model zoo reports for its checkpoints ("using CLIP as feature extractor instead of Inception" for FFHQ).  The reference ships
no evaluation script; this one has no counterpart there.

    python scripts/rdm_eval.py --real DIR --fake DIR --clip_ckpt ViT-B-32.pt --gpu 0

prints ONE JSON line: {"fid", "precision", "recall", "n_real", "n_gen", "k", "features", "normalized"}.  The features are the tower's un-normalised
pooled embedding (--normalize divides each by its norm).  Two more metrics on request, for the sets the first three are weak on:

    --kid [--kid_subsets 100 --kid_subset_size 1000 --kid_seed 0]    adds "kid", "kid_std" (and the three settings): Kernel Inception Distance
                (Binkowski et al. 2018) on the same features, mean and std over the subsets; unbiased at any set size, where FID is not
    --density_coverage [--dc_k 5]                                     adds "density", "coverage", "dc_k" (Naeem et al. 2020): density does not
                saturate at 1 as precision does, coverage is the recall that generated outliers cannot inflate  --synthetic runs on the seeded synthetic CLIP weights: the numbers then measure
nothing about image quality, the path runs without checkpoint files.
"""
import argparse
import json
import os
import sys
from pathlib import Path

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IMAGE_SUFFIXES = (".png", ".jpg", ".jpeg", ".bmp", ".webp")


def build_parser() -> argparse.ArgumentParser:
    parser = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    parser.add_argument("--real", type=Path, required=True, help="folder of real images")
    parser.add_argument("--fake", type=Path, required=True, help="folder of generated images")
    parser.add_argument("--clip_ckpt", type=Path, default=None, help="CLIP ViT-B/32 state_dict (.pt)")
    parser.add_argument("--gpu", type=int, default=0, help="on which gpu to run")
    parser.add_argument("--k", type=int, default=3, help="neighbour rank of the precision / recall balls (1..8)")
    parser.add_argument("--batch_size", type=int, default=64, help="images per CLIP forward")
    parser.add_argument("--normalize", default=False, action="store_true", help="L2-normalise the features (default: un-normalised)")
    parser.add_argument("--synthetic", default=False, action="store_true", help="seeded synthetic CLIP weights instead of --clip_ckpt")
    parser.add_argument("--kid", default=False, action="store_true", help="also report KID (mean and std over subsets)")
    parser.add_argument("--kid_subsets", type=int, default=100, help="subsets KID averages over (0: one estimate on the whole sets)")
    parser.add_argument("--kid_subset_size", type=int, default=1000, help="rows per KID subset (clamped to the smaller set)")
    parser.add_argument("--kid_seed", type=int, default=0, help="seed of the subset draw")
    parser.add_argument("--density_coverage", default=False, action="store_true", help="also report density and coverage")
    parser.add_argument("--dc_k", type=int, default=5, help="neighbour rank of the density / coverage balls (1..8)")
    return parser


def parse_args(argv=None) -> argparse.Namespace:
    parser = build_parser()
    opt = parser.parse_args(argv)
    if not 1 <= opt.k <= 8:
        parser.error(f"--k must lie in 1..8, got {opt.k}")
    if not 1 <= opt.dc_k <= 8:
        parser.error(f"--dc_k must lie in 1..8, got {opt.dc_k}")
    if opt.kid_subsets < 0:
        parser.error(f"--kid_subsets must be 0 (the whole sets) or more, got {opt.kid_subsets}")
    if opt.kid_subset_size < 2:
        parser.error(f"--kid_subset_size must be at least 2 (the unbiased estimate leaves the diagonal out), got {opt.kid_subset_size}")
    if opt.batch_size < 1:
        parser.error(f"--batch_size must be positive, got {opt.batch_size}")
    if opt.gpu < 0:
        parser.error("--gpu must name a device: the native library has no CPU path")
    if opt.clip_ckpt is None and not opt.synthetic:
        parser.error("pass --clip_ckpt <ViT-B/32 state_dict>, or --synthetic for the seeded synthetic weights")
    return opt


def extras(opt):
    """The `extra` of rdm_amd.metrics.evaluate that the flags ask for."""
    return tuple(name for name, on in (("kid", opt.kid), ("density_coverage", opt.density_coverage)) if on)


def list_images(folder):
    paths = sorted(p for p in Path(folder).iterdir() if p.suffix.lower() in IMAGE_SUFFIXES)
    if not paths:
        raise SystemExit(f"rdm_eval.py: no images ({', '.join(IMAGE_SUFFIXES)}) in {folder}")
    return paths


def image_batches(paths, batch_size):
    """Yields f32 [b, 3, H, W] in [-1, 1]; images of one batch must share a size (a new batch starts where the size changes)."""
    import numpy as np
    import torch
    from PIL import Image
    batch, size = [], None
    for p in paths:
        img = np.asarray(Image.open(p).convert("RGB"), dtype=np.float32)
        if batch and (img.shape != size or len(batch) == batch_size):
            yield torch.from_numpy(np.stack(batch)).permute(0, 3, 1, 2).contiguous()
            batch = []
        size = img.shape
        batch.append(img / 127.5 - 1.0)
    if batch:
        yield torch.from_numpy(np.stack(batch)).permute(0, 3, 1, 2).contiguous()


def main(argv=None):
    opt = parse_args(argv)
    sys.path.insert(0, ROOT)
    import torch
    import rdm_amd  # noqa: F401
    from rdm_amd import _lib, metrics, synthetic
    from rdm_amd.modules.retrievers import ClipImageRetriever
    torch.set_grad_enabled(False)
    ctx = _lib.Context(opt.gpu)
    sd = synthetic.clip_state_dict(_lib.make_clip_cfg()) if opt.synthetic else torch.load(opt.clip_ckpt, map_location="cpu")
    model = ClipImageRetriever(state_dict=sd, ctx=ctx)
    res = metrics.evaluate(model, image_batches(list_images(opt.real), opt.batch_size), image_batches(list_images(opt.fake), opt.batch_size),
                           k=opt.k, batch=opt.batch_size, normalize=opt.normalize, extra=extras(opt), kid_subsets=opt.kid_subsets,
                           kid_subset_size=opt.kid_subset_size, kid_seed=opt.kid_seed, dc_k=opt.dc_k)
    res.update(k=opt.k, features="clip-vit-b32-synthetic" if opt.synthetic else "clip-vit-b32", normalized=bool(opt.normalize))
    if opt.kid:
        res.update(kid_subsets=opt.kid_subsets, kid_subset_size=opt.kid_subset_size, kid_seed=opt.kid_seed)
    if opt.density_coverage:
        res.update(dc_k=opt.dc_k)
    print(json.dumps(res))
    ctx.close()
    return res


if __name__ == "__main__":
    main()
