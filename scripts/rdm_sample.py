#!/usr/bin/env python3
"""Native counterpart of the reference's scripts/rdm_sample.py.

Every flag of the reference parser (scripts/rdm_sample.py:22-143) is kept with the same spelling, type, default and
meaning: -s/--savepath, --gpu, --model_path, --save_nns, -bs/--batch_size, -n/--n_runs, --seed, --increase_guidance,
--keep_qids, --guidance_scale, --top_m, --k_nn, --steps, -c/--caption, --only_caption, --omit_query, --unconditional,
--use_weights.  The run loops follow :225-315: caption == "" -> sample_from_rdata, else CLIP-encode the caption once and
sample_with_query; `seed_everything(seed)` before EVERY run; DDIM with the sampler's default eta (0.0, deterministic);
k_nn = 1 with --only_caption; omit_query masked by only_caption; `--increase_guidance` adds 1.0 after each run; files are
`{sampling_start}-{key}-run{n}-sample{i}.png` with a `%Y-%m-%d-%H-%M-%S` stamp; uint8 conversion truncates (:203-214).

Deliberate differences:
  * `--seed N` works (the reference dereferences a non-existent `opt.r_runs`, :141);
  * `--gpu -1` (the reference's default, "none") is refused: the native library has no CPU path;
  * `--save_nns` raises NotImplementedError (needs the raw OpenImages JPEGs behind `get_nn_patches`);
  * retrieval is the exact brute-force search on the GPU instead of ScaNN's approximate index.
Additions (not in the reference, all optional): `--clip_ckpt` (CLIP ViT-B/32 state_dict; the reference downloads it),
`--synthetic` (seeded random weights and database: the 6.2 GB checkpoint / 18 GB database are unreachable without a
network), `--gpus N` (batch-sharded multi-GPU sampling, one process per GPU via torch.distributed.run, RCCL all-gather of
the finished images; `--gpu` is then ignored and each rank uses its LOCAL_RANK), `--plms` (sample with ldm's PLMSSampler on
`--steps` instead of DDIM: same schedule, about half the steps for the same accuracy; works with `--gpus N`), `--dpm_solver`
(sample with DPM-Solver++(2M), ldm's DPMSolverSampler, on a logSNR grid of at most `--steps` steps: 15-25 steps under guidance;
works with `--gpus N`; not together with `--plms`), `--uni_pc` (sample with UniPC order 2: DPM-Solver++(2M) plus a corrector that costs no
forward, on the same grid; works with `--gpus N`; not together with `--plms` or `--dpm_solver`), `--dpm_solver_sde` (sample with
SDE-DPM-Solver++(2M): DPM-Solver++'s grid and step counts with fresh noise at every step, so a stochastic sampler in about 20 forwards; works with
`--device_noise` and `--gpus N`; not together with the other sampler flags), `--height PX` / `--width PX` (image size in pixels, default the model's own: the UNet and
the first stage are convolutional, so a model samples at other sizes -- the reference reaches this through `sample_log(custom_shape=)`
only, its script has no flag; multiples of 32 = first-stage factor 4 x UNet down factor 8 of the shipped models; every sampler, and
`--gpus N`), `--eta FLOAT` (DDIM's eta, default 0.0 = the reference script's deterministic DDIM; above 0 every step adds
sigma_t-scaled noise; DDIM only, PLMS refuses it and DPM-Solver++ / UniPC ignore it), `--device_noise` (the starting latents and the
`--eta` noise come from the library's counter-based generator inside the step kernels, keyed by (the run's seed draw, global sample
index): no noise tensor is drawn or stacked in Python, and the images differ from the default torch-generator streams; works with
`--gpus N` with the same sharding invariance), `--init_img PATH_OR_DIR` / `--strength S` / `--invert` (image-to-image on DDIM: the image,
resized to the model's size or `--height` / `--width`, is encoded by the first stage and either noised to `int(S x steps)` steps up the
schedule or, with `--invert`, taken there by deterministic DDIM inversion, then decoded under the retrieved neighbours; strength 1.0 runs
every step; works with `--gpus N` and `--device_noise`; not with `--plms` / `--dpm_solver` / `--uni_pc` / `--dpm_solver_sde`),
`--mask PNG` (inpainting, with `--init_img`: a grey image, WHITE = REPAINT, resized to the call's size; the white region is sampled
anew under the retrieved neighbours and the black region keeps the init image -- in the native DDIM loop, so it works with `--strength`,
`--eta`, `--device_noise` and `--gpus N`; not with `--invert` or the multistep samplers).
"""
import argparse
import datetime
import os
import random
import subprocess
import sys
from pathlib import Path

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_parser() -> argparse.ArgumentParser:
    parser = argparse.ArgumentParser()
    parser.add_argument("-s", "--savepath", type=Path, default="out/rdm", help="Path to savedir")
    parser.add_argument("--gpu", type=int, default=-1, help="On which gpu to sample, -1 for none")
    parser.add_argument("--model_path", type=Path, default="models/rdm/imagenet", help="Path to pretrained model")
    parser.add_argument("--save_nns", default=False, action="store_true", help="Save nearest neighbors")
    parser.add_argument("-bs", "--batch_size", type=int, default=4, help="How many images to generate at once")
    parser.add_argument("-n", "--n_runs", type=int, default=2, help="repeat sampling this number of times")
    parser.add_argument("--seed", type=int, default=None, help="Seed each iteration")
    parser.add_argument("--increase_guidance", default=False, action="store_true", help="Increase cfg after each iteration")
    parser.add_argument("--keep_qids", default=False, action="store_true", help="Keep same queries for each run")
    parser.add_argument("--guidance_scale", type=float, default=2., help="classifier free (transformer) guidance")
    parser.add_argument("--top_m", type=float, default=0.01, help="top-m sampling")
    parser.add_argument("--k_nn", type=int, default=4, help="number of neighbors drawn for sampling")
    parser.add_argument("--steps", type=int, default=100, help="number of ddim steps")
    parser.add_argument("-c", "--caption", type=str, default="", help="Caption used for neighbor retrieval")
    parser.add_argument("--only_caption", default=False, action="store_true", help="use the caption only, no neighbors")
    parser.add_argument("--omit_query", default=False, action="store_true", help="Omit the caption query as nearest neighbor itself")
    parser.add_argument("--unconditional", default=False, action="store_true",
                        help="Sample 'unconditonal' as in the unconditional part of cfg")    # parsed, never read (as in the reference)
    parser.add_argument("--use_weights", default=False, action="store_true",
                        help="Use proposal distribution weights (else sample uniform under top_m)")
    # ---- additions of the native counterpart
    parser.add_argument("--clip_ckpt", type=Path, default=None, help="[native] CLIP ViT-B/32 state_dict (.pt)")
    parser.add_argument("--synthetic", default=False, action="store_true",
                        help="[native] seeded random weights + synthetic database instead of checkpoint files")
    parser.add_argument("--synthetic_db_rows", type=int, default=200_000, help="[native] rows of the --synthetic database")
    parser.add_argument("--gpus", type=int, default=1, help="[native] shard each batch over this many GPUs (RCCL)")
    parser.add_argument("--shard_db", action="store_true", help="[native] with --gpus N: shard the database ROWS over the GPUs instead of "
                        "replicating them (databases beyond one GPU's memory); neighbours are merged in one exchange per search")
    parser.add_argument("--plms", default=False, action="store_true", help="[native] sample with PLMS (ldm PLMSSampler) instead of DDIM")
    parser.add_argument("--dpm_solver", default=False, action="store_true",
                        help="[native] sample with DPM-Solver++(2M) (ldm DPMSolverSampler) on a logSNR grid instead of DDIM")
    parser.add_argument("--height", type=int, default=None, help="[native] image height in pixels (default: the model's own size); a multiple of 32")
    parser.add_argument("--width", type=int, default=None, help="[native] image width in pixels (default: the model's own size); a multiple of 32")
    parser.add_argument("--uni_pc", default=False, action="store_true",
                        help="[native] sample with UniPC (order 2, bh2, with the corrector) on a logSNR grid instead of DDIM")
    parser.add_argument("--dpm_solver_sde", default=False, action="store_true",
                        help="[native] sample with SDE-DPM-Solver++(2M) on a logSNR grid instead of DDIM: fresh noise every step, at DPM-Solver++'s "
                        "step counts")
    parser.add_argument("--eta", type=float, default=0.0, help="[native] DDIM eta (0.0: deterministic DDIM, as the reference script samples)")
    parser.add_argument("--device_noise", default=False, action="store_true",
                        help="[native] starting latents and per-step noise from the library's counter-based generator inside the step kernels "
                        "(no noise stack)")
    parser.add_argument("--init_img", type=Path, default=None,
                        help="[native] image-to-image: start from this image (or the images of this directory: one, or one per sample of the "
                        "batch) instead of pure noise; DDIM only")
    parser.add_argument("--strength", type=float, default=0.75,
                        help="[native] with --init_img: how far up the schedule the image is taken, in (0, 1]; 1.0 runs every step")
    parser.add_argument("--invert", default=False, action="store_true",
                        help="[native] with --init_img: start from the image's deterministic DDIM inversion instead of noising it")
    parser.add_argument("--mask", type=Path, default=None,
                        help="[native] with --init_img: inpainting -- a grey PNG, white = repaint, black = keep the init image; DDIM only, "
                        "not with --invert")
    parser.add_argument("--db_subset", type=Path, default=None,
                        help="[native] retrieve neighbours from a subset of the database only: a .npy file holding an integer array of row "
                        "indices or a boolean array over all rows (a class, a style, a held-out split, a deny list); works with --gpus N "
                        "and --shard_db")
    parser.add_argument("--db_subset_invert", default=False, action="store_true",
                        help="[native] with --db_subset: retrieve from every row NOT in the file")
    parser.add_argument("--nn_counts", type=nn_counts_arg, default=None,
                        help="[native] how many entries of its conditioning a sample attends, in [1, k_nn]: one value, or one per sample of "
                        "the batch, e.g. 4,2,1,1 (the rest are masked in the UNet's cross-attention)")
    parser.add_argument("--short_subsets", type=str, default="error", choices=("error", "mask"),
                        help="[native] with --db_subset: a subset of fewer rows than --k_nn asks for is an error (default), or its missing "
                        "neighbours are masked")
    return parser


def nn_counts_arg(text: str):
    """--nn_counts: '3' -> 3, '4,2,1' -> [4, 2, 1]"""
    try:
        vals = [int(v) for v in text.split(",")]
    except ValueError:
        raise argparse.ArgumentTypeError(f"expected an integer or a comma-separated list of integers, got {text!r}")
    if not vals or min(vals) < 1:
        raise argparse.ArgumentTypeError(f"neighbour counts are at least 1, got {text!r}")
    return vals[0] if len(vals) == 1 else vals


SIZE_MULTIPLE = 32          # first-stage factor (VQ-f4: 4) x UNet down factor (8) of the shipped models


def parse_args(argv=None) -> argparse.Namespace:
    parser = build_parser()
    opt = parser.parse_args(argv)
    for name in ("height", "width"):
        v = getattr(opt, name)
        if v is not None and (v < SIZE_MULTIPLE or v % SIZE_MULTIPLE):
            parser.error(f"--{name} must be a positive multiple of {SIZE_MULTIPLE} (first-stage factor x UNet down factor), got {v}")
    if opt.init_img is not None:
        for name in ("plms", "dpm_solver", "uni_pc", "dpm_solver_sde"):
            if getattr(opt, name):
                parser.error(f"--init_img runs on the DDIM sampler only: drop --{name}")
        if not 0.0 < opt.strength <= 1.0:
            parser.error(f"--strength must lie in (0, 1], got {opt.strength}")
    elif opt.invert:
        parser.error("--invert needs --init_img")
    if opt.mask is not None:
        if opt.init_img is None:
            parser.error("--mask needs --init_img (the image whose black-masked region is kept)")
        if opt.invert:
            parser.error("--mask starts from the noised image: drop --invert")
    if opt.db_subset_invert and opt.db_subset is None:
        parser.error("--db_subset_invert needs --db_subset")
    if opt.short_subsets != "error" and opt.db_subset is None:
        parser.error("--short_subsets needs --db_subset")
    if isinstance(opt.nn_counts, list) and len(opt.nn_counts) != opt.batch_size:
        parser.error(f"--nn_counts takes one value or one per sample of the batch ({opt.batch_size}), got {len(opt.nn_counts)}")
    k_eff = 1 if opt.only_caption else opt.k_nn
    if opt.nn_counts is not None and max(opt.nn_counts if isinstance(opt.nn_counts, list) else [opt.nn_counts]) > k_eff:
        parser.error(f"--nn_counts must lie in [1, {k_eff}] (the neighbours the call retrieves)")
    if opt.top_m > 1.0:
        opt.top_m = int(opt.top_m)          # top_m should be int if a fixed number of images is given (:138-140)
    if opt.seed is not None and (not opt.increase_guidance) and opt.n_runs > 1:
        print("Warning: You will get the same images each run")
    return opt


def seed_everything(seed: int):
    """pytorch_lightning.seed_everything (rdm_sample.py:14, 235, 281): python, numpy and torch (all devices) RNGs."""
    import torch
    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)
    if torch.cuda.is_available():
        torch.cuda.manual_seed_all(seed)
    return seed


def custom_to_pil(x):
    """rdm_sample.py:203-214: clamp(-1,1) -> (x+1)/2 -> HWC -> (255 x).astype(uint8), i.e. truncation."""
    import torch
    from PIL import Image
    if isinstance(x, np.ndarray):
        x = torch.from_numpy(x)
    x = x.detach().cpu()
    x = torch.clamp(x, -1., 1.)
    x = (x + 1.) / 2.
    x = x.permute(1, 2, 0).numpy()
    x = (255 * x).astype(np.uint8)
    x = Image.fromarray(x)
    if not x.mode == "RGB":
        x = x.convert("RGB")
    return x


def save_image(x, savename: str):
    custom_to_pil(x).save(savename)


def load_model(opt: argparse.Namespace):
    """rdm_sample.py:146-187: config.yaml + model.ckpt -> MinimalRETRODiffusion on the selected GPU (EMA weights resident in
    HBM), retriever = DatasetBuilder over the saved embeddings with the CLIP towers on the same device."""
    import torch
    import rdm_amd  # noqa: F401
    from rdm_amd import _lib, synthetic
    from rdm_amd.data.retrieval_dataset.dsetbuilder import DatasetBuilder
    from rdm_amd.models.diffusion.ddpm import MinimalRETRODiffusion
    from rdm_amd.modules.retrievers import ClipImageRetriever

    if opt.save_nns:
        raise NotImplementedError("--save_nns needs the raw OpenImages patches behind get_nn_patches (out of scope, SURVEY.md §2 #8)")
    if opt.gpu < 0:
        raise SystemExit("rdm_sample.py (native): --gpu must name a HIP device; the native library has no CPU path")
    if opt.synthetic:
        model = MinimalRETRODiffusion(unet_config={"params": {}}, first_stage_config={"params": {"ddconfig": {}}}, k_nn=4, device=opt.gpu)
        model.load_unet_state_dict(synthetic.unet_state_dict(model.unet_cfg))
        fsd = synthetic.vq_state_dict(model.vq_cfg)
        if getattr(opt, "init_img", None) is not None:                  # image-to-image encodes the image: the first stage's other half
            fsd.update(synthetic.vq_encoder_state_dict(model.vq_cfg))
        model.load_first_stage_state_dict(fsd)
        n = opt.synthetic_db_rows
        pool = {"embedding": synthetic.clip_like_rows(n), "img_id": np.arange(n), "patch_coords": np.zeros((n, 4), np.int64)}
        retr = ClipImageRetriever(state_dict=synthetic.clip_state_dict(_lib.make_clip_cfg()), ctx=model.ctx)
        model.retriever = DatasetBuilder(data_pool=pool, retriever=retr, ctx=model.ctx)
        model.nn_memory = torch.arange(min(10_000, n)); model.use_memory = True
        return model.eval()
    import yaml
    model_dir = opt.model_path
    config_path, ckpt_path = model_dir / "config.yaml", model_dir / "model.ckpt"
    assert config_path.is_file(), f"Did not found config at {config_path}"
    assert ckpt_path.is_file(), f"Did not found ckpt at {ckpt_path}"
    cfg = yaml.safe_load(open(config_path))["model"]["params"]
    pl_sd = torch.load(ckpt_path, map_location="cpu")
    rp = dict(cfg["retrieval_cfg"]["params"])
    nn_memory = cfg.get("nn_memory")
    if isinstance(nn_memory, str) and os.path.isfile(nn_memory):          # ddpm.py:168-176: pickled {'nn_memory', 'id_count'}
        import pickle
        with open(nn_memory, "rb") as f:
            mem = pickle.load(f)
        nn_memory, id_count = mem["nn_memory"], mem.get("id_count")
    else:
        nn_memory, id_count = None, None
    model = MinimalRETRODiffusion(unet_config=cfg["unet_config"], first_stage_config=cfg["first_stage_config"], k_nn=cfg.get("k_nn", 4),
                                  timesteps=cfg.get("timesteps", 1000), linear_start=cfg["linear_start"], linear_end=cfg["linear_end"],
                                  image_size=cfg["image_size"], channels=cfg["channels"], log_every_t=cfg.get("log_every_t", 200),
                                  scale_factor=cfg.get("scale_factor", 1.0), nn_memory=nn_memory, id_count=id_count, device=opt.gpu)
    m, u = model.load_state_dict(pl_sd["state_dict"], strict=False)
    print("Loaded model.")
    clip_sd = torch.load(opt.clip_ckpt, map_location="cpu") if opt.clip_ckpt else None
    if clip_sd is None:
        raise SystemExit("rdm_sample.py (native): pass --clip_ckpt <ViT-B/32 state_dict>; the reference downloads it (no network here)")
    retr = ClipImageRetriever(model=rp.get("retriever_config", {}).get("params", {}).get("model", "ViT-B/32"), state_dict=clip_sd, ctx=model.ctx)
    model.retriever = DatasetBuilder(saved_embeddings=rp["saved_embeddings"], k=rp.get("k", 20), retriever=retr, ctx=model.ctx,
                                     load_patch_dataset=False)
    return model.eval()


def _save_logs(logs, keys, opt, sampling_start, n):
    for key in logs:
        if keys is not None and key not in keys:
            continue
        for bi, be in enumerate(logs[key]):
            savename = os.path.join(opt.savepath, f'{sampling_start}-{key}-run{n}-sample{bi}.png')
            if be.ndim == 3:
                save_image(be, savename)
            else:
                raise NotImplementedError("image grids (batched_nns) belong to --save_nns")


def _sampler_kwargs(opt: argparse.Namespace, model=None) -> dict:
    """--plms / --dpm_solver / --uni_pc / --dpm_solver_sde / --height / --width / --eta reach MinimalRETRODiffusion.sample_log (the sizes as its custom_shape, in
    latent pixels), --device_noise sample_with_query / sample_from_rdata; without them the calls are the reference's."""
    kw = {name: True for name in ("plms", "dpm_solver", "uni_pc", "dpm_solver_sde", "device_noise") if getattr(opt, name, False)}
    if getattr(opt, "eta", 0.0) != 0.0:
        kw["eta"] = opt.eta
    height, width = getattr(opt, "height", None), getattr(opt, "width", None)
    if height is not None or width is not None:
        f = 1 << (model.vq_cfg.n_ch_mult - 1)                       # pixels per latent pixel
        own = model.image_size * f
        height, width = (own if height is None else height), (own if width is None else width)
        if height % f or width % f:
            raise SystemExit(f"rdm_sample.py (native): --height / --width must be multiples of the first stage's factor {f}")
        kw["custom_shape"] = (model.channels, height // f, width // f)       # checked against the UNet's down factor by the model
    if getattr(opt, "init_img", None) is not None:
        kw.update(init_image=load_init_images(opt, model, kw.get("custom_shape")), strength=opt.strength)
        if opt.invert:
            kw["invert"] = True
    if getattr(opt, "mask", None) is not None:
        kw["inpaint_mask"] = load_inpaint_mask(opt, model, kw.get("custom_shape"))
    if getattr(opt, "db_subset", None) is not None:
        kw["db_subset"] = define_db_subset(opt, model)
    if getattr(opt, "nn_counts", None) is not None:
        kw["nn_counts"] = opt.nn_counts
    if getattr(opt, "short_subsets", "error") != "error":
        kw["short_subsets"] = opt.short_subsets
    return kw


DB_SUBSET_NAME = "--db_subset"


def define_db_subset(opt: argparse.Namespace, model) -> str:
    """--db_subset / --db_subset_invert: the .npy index or boolean array becomes a named subset of the model's retriever (built once,
    per shard under --shard_db) -> the name sample_with_query / sample_from_rdata take as db_subset."""
    if DB_SUBSET_NAME not in model.retriever.subsets():
        n = len(model.retriever.data_pool["embedding"])
        rows = np.load(opt.db_subset, allow_pickle=False)
        if rows.dtype != np.bool_ and not np.issubdtype(rows.dtype, np.integer):
            raise SystemExit(f"rdm_sample.py (native): --db_subset must hold an integer index array or a boolean array, got {rows.dtype}")
        if rows.dtype != np.bool_:
            if rows.size and (rows.min() < 0 or rows.max() >= n):
                raise SystemExit(f"rdm_sample.py (native): --db_subset holds row indices outside the database's [0, {n})")
            member = np.zeros(n, dtype=np.bool_)
            member[rows.reshape(-1)] = True
            rows = member
        elif rows.shape != (n,):
            raise SystemExit(f"rdm_sample.py (native): a boolean --db_subset must have one entry per database row ({n}), got {rows.shape}")
        model.retriever.define_subset(DB_SUBSET_NAME, ~rows if opt.db_subset_invert else rows)
    return DB_SUBSET_NAME


def load_inpaint_mask(opt: argparse.Namespace, model, custom_shape=None):
    """--mask: the grey PNG at the call's size in pixels (resized like the init image), WHITE = REPAINT -> f32 [1, H, W] in [0, 1] with
    1 = keep, the convention of sample_with_query's inpaint_mask: 1 - mask / 255.  The model averages it down to latent pixels."""
    import torch
    from PIL import Image
    f = 1 << (model.vq_cfg.n_ch_mult - 1)
    _, h, w = custom_shape if custom_shape is not None else (model.channels, model.image_size, model.image_size)
    grey = Image.open(opt.mask).convert("L").resize((w * f, h * f), Image.BILINEAR)
    return (1.0 - torch.from_numpy(np.asarray(grey, dtype=np.float32)) / 255.0)[None].contiguous()


def load_init_images(opt: argparse.Namespace, model, custom_shape=None):
    """--init_img: the image file, or a directory's images (one, repeated by the model, or one per sample of the batch), with the loader
    of rarm_sample.py --complete_from at the call's size in pixels -> f32 [n,H,W,3] in [-1,1], as sample_with_query takes init_image."""
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from rarm_sample import load_images
    f = 1 << (model.vq_cfg.n_ch_mult - 1)
    _, h, w = custom_shape if custom_shape is not None else (model.channels, model.image_size, model.image_size)
    images = load_images(opt.init_img, h * f, w * f)
    if images.shape[0] not in (1, opt.batch_size):
        raise SystemExit(f"rdm_sample.py (native): --init_img gives {images.shape[0]} images; give one, or one per sample of -bs {opt.batch_size}")
    return images.permute(0, 2, 3, 1).contiguous()


def sample_unconditional(model, opt: argparse.Namespace, is_writer=True):
    """rdm_sample.py:225-266."""
    qids = model.get_qids(opt.top_m, opt.batch_size, use_weights=opt.use_weights) if opt.keep_qids else None
    sampling_start = datetime.datetime.now().strftime("%Y-%m-%d-%H-%M-%S")
    for n in range(opt.n_runs):
        if opt.seed is not None:
            seed_everything(opt.seed)
        print("Sampling query and neighbors (wait for the sampling to start)")
        logs = model.sample_from_rdata(opt.batch_size, qids=qids, k_nn=opt.k_nn, return_nns=opt.save_nns, use_weights=opt.use_weights,
                                       memsize=opt.top_m, unconditional_guidance_scale=opt.guidance_scale, ddim_steps=opt.steps,
                                       ddim=True, unconditional_retro_guidance_label=0., **_sampler_kwargs(opt, model))
        if is_writer:
            _save_logs(logs, ["samples_with_sampled_nns", "batched_nns"], opt, sampling_start, n)
        if opt.increase_guidance:
            opt.guidance_scale += 1.0
            print(f"New guidance scale: {opt.guidance_scale}")
    print("Done")
    return sampling_start


def sample_conditional(model, opt: argparse.Namespace, is_writer=True):
    """rdm_sample.py:270-315."""
    from rdm_amd.modules.custom_clip.tokenizer import tokenize
    import torch
    sampling_start = datetime.datetime.now().strftime("%Y-%m-%d-%H-%M-%S")
    tokenized = torch.from_numpy(tokenize([opt.caption] * opt.batch_size))
    clip = model.retriever.retriever.model
    query_embeddings = clip.encode_text(tokenized).cpu()
    del tokenized
    for n in range(opt.n_runs):
        if opt.seed is not None:
            seed_everything(opt.seed)
        print("Sampling query and neighbors (wait for the sampling to start)")
        logs = model.sample_with_query(query=query_embeddings, query_embedded=True, k_nn=opt.k_nn if not opt.only_caption else 1,
                                       return_nns=opt.save_nns and not opt.only_caption, visualize_nns=opt.save_nns and not opt.only_caption,
                                       use_weights=opt.use_weights, unconditional_guidance_scale=opt.guidance_scale, ddim_steps=opt.steps,
                                       ddim=True, unconditional_retro_guidance_label=0., omit_query=opt.omit_query and not opt.only_caption,
                                       **_sampler_kwargs(opt, model))
        print(f"Run {n + 1}/{opt.n_runs}")
        if is_writer:
            _save_logs(logs, None, opt, sampling_start, n)
        if opt.increase_guidance:
            opt.guidance_scale += 1.0
            print(f"New guidance scale: {opt.guidance_scale}")
    print("Done")
    return sampling_start


def main(argv=None):
    opt = parse_args(argv)
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if opt.gpus > 1 and world == 1:
        # one process per GPU; launched BEFORE anything in this process touches the GPU (importing the package / torch does not);
        # refused under a profiler, where the preloaded tool already has (rdm_amd.parallel.safe_self_launch)
        sys.path.insert(0, ROOT)
        import rdm_amd  # noqa: F401
        from rdm_amd import parallel
        sys.exit(parallel.safe_self_launch(__file__, opt.gpus, sys.argv[1:] if argv is None else list(argv)))
    sys.path.insert(0, ROOT)
    opt.savepath.mkdir(parents=True, exist_ok=True)
    is_writer = True
    if world > 1:
        from rdm_amd import parallel
        rank, local = parallel.init_distributed()
        opt.gpu = local
        is_writer = rank == 0
    model = load_model(opt)
    if world > 1:
        model.set_distributed(True, shard_db=opt.shard_db)       # noise streams: f(shared seed drawn after seed_everything, global row)
    if opt.caption == "":
        sample_unconditional(model, opt, is_writer)
    else:
        sample_conditional(model, opt, is_writer)
    if world > 1:
        from rdm_amd import parallel
        parallel.shutdown()


if __name__ == "__main__":
    main()
