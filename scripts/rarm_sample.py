#!/usr/bin/env python3
"""Native counterpart of the reference's scripts/rarm_sample.py (RARM: retrieval-augmented autoregressive sampling).

Same flags, defaults and run loop as scripts/rarm_sample.py:100-293: -s/--savepath (out/rarm), --gpu, --model_path
(models/rarm/imagenet/dogs), --save_nns, -bs, -n, --seed, --increase_guidance, --keep_qids, --guidance_scale (1.0), --top_k (256),
--temperature (1.0), --top_m (0.01), --k_nn (4), -c/--caption, --only_caption, --unconditional, --use_weights; 256 tokens
(f16 first stage), `seed_everything` before every run, files `{start}-{key}-run{n}-sample{i}.png`.
Deliberate differences: as scripts/rdm_sample.py (no CPU path, --save_nns unsupported, --seed works).  Additions:
--clip_ckpt, --synthetic, --top_p (1.0: nucleus sampling after top-k, the `top_p` the reference's sampling_util names and asserts away),
--complete_from PATH [--keep_rows R]: image completion as LatentImageRETRO.log_images does it (`samples_half`, transformer.py:457-462) --
every image of PATH (a file or a directory) is centre-cropped, resized to the first-stage resolution and encoded to its VQGAN codes, the
first R code rows (default: half the grid) are kept and the rest is sampled with the flags above; neighbours come from the image's own
CLIP embedding unless -c / --only_caption / --unconditional say otherwise.  Writes `{start}-samples_half-run{n}-sample{i}.png` and
`{start}-reconstructions-run{n}-sample{i}.png`.
--prefill (with --complete_from only): the kept codes are fed to the transformer in one whole-sequence pass instead of token by token.
--score PATH: no sampling -- every image of PATH is encoded, its neighbours retrieved as --complete_from does, and its teacher-forced
negative log-likelihood under them (LatentImageRETRO.validation_step, transformer.py:65-70) is printed: one line per image with the mean
in nats and bits per code, then the mean over all images as the reference's `val/loss`.
"""
import argparse
import datetime
import os
import sys
from pathlib import Path

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
sys.path.insert(0, ROOT)
from rdm_sample import custom_to_pil, save_image, seed_everything  # noqa: E402,F401


def build_parser() -> argparse.ArgumentParser:
    parser = argparse.ArgumentParser()
    parser.add_argument("-s", "--savepath", type=Path, default="out/rarm", help="Path to savedir")
    parser.add_argument("--gpu", type=int, default=-1, help="On which gpu to sample, -1 for none")
    parser.add_argument("--model_path", type=Path, default="models/rarm/imagenet/dogs", help="Path to pretrained model")
    parser.add_argument("--save_nns", default=False, action="store_true", help="Save nearest neighbors")
    parser.add_argument("-bs", "--batch_size", type=int, default=4, help="How many images to generate at once")
    parser.add_argument("-n", "--n_runs", type=int, default=2, help="repeat sampling this number of times")
    parser.add_argument("--seed", type=int, default=None, help="Seed each iteration")
    parser.add_argument("--increase_guidance", default=False, action="store_true", help="Increase cfg after each iteration")
    parser.add_argument("--keep_qids", default=False, action="store_true", help="Keep same queries for each run")
    parser.add_argument("--guidance_scale", type=float, default=1., help="classifier free (transformer) guidance")
    parser.add_argument("--top_k", type=int, default=256, help="top-k sampling")
    parser.add_argument("--top_p", type=float, default=1.0, help="[native] top-p (nucleus) sampling after top-k, in (0, 1] (default: 1.0, off)")
    parser.add_argument("--temperature", type=float, default=1., help="temperature sampling")
    parser.add_argument("--top_m", type=float, default=0.01, help="top-m sampling")
    parser.add_argument("--k_nn", type=int, default=4, help="number of neighbors drawn for sampling")
    parser.add_argument("-c", "--caption", type=str, default="", help="Caption used for neighbor retrieval")
    parser.add_argument("--only_caption", default=False, action="store_true", help="use the caption only, no neighbors")
    parser.add_argument("--unconditional", default=False, action="store_true",
                        help="Sample 'unconditonal' as in the unconditional part of cfg")
    parser.add_argument("--use_weights", default=False, action="store_true",
                        help="Use proposal distribution weights (else sample uniform under top_m)")
    parser.add_argument("--clip_ckpt", type=Path, default=None, help="[native] CLIP ViT-B/32 state_dict (.pt)")
    parser.add_argument("--synthetic", default=False, action="store_true", help="[native] seeded random weights + synthetic database")
    parser.add_argument("--synthetic_db_rows", type=int, default=200_000, help="[native] rows of the --synthetic database")
    parser.add_argument("--complete_from", type=Path, default=None,
                        help="[native] image file or directory: keep the first code rows of each image and sample the rest")
    parser.add_argument("--keep_rows", type=int, default=None, help="[native] code rows kept by --complete_from (default: half the grid)")
    parser.add_argument("--prefill", default=False, action="store_true",
                        help="[native] feed the codes kept by --complete_from in one whole-sequence pass instead of token by token")
    parser.add_argument("--score", type=Path, default=None,
                        help="[native] image file or directory: print each image's mean negative log-likelihood per code, sample nothing")
    return parser


def parse_args(argv=None) -> argparse.Namespace:
    opt = build_parser().parse_args(argv)
    if opt.top_m > 1.0:
        opt.top_m = int(opt.top_m)
    if opt.prefill and opt.complete_from is None:
        print("Warning: --prefill only has an effect with --complete_from")
    if opt.seed is not None and (not opt.increase_guidance) and opt.n_runs > 1:
        print("Warning: You will get the same images each run")
    return opt


def load_model(opt):
    """rarm_sample.py:25-70."""
    import torch
    import rdm_amd  # noqa: F401
    from rdm_amd import _lib, synthetic
    from rdm_amd.data.retrieval_dataset.dsetbuilder import DatasetBuilder
    from rdm_amd.models.autoregression.transformer import LatentImageRETRO
    from rdm_amd.modules.retrievers import ClipImageRetriever
    if opt.save_nns:
        raise NotImplementedError("--save_nns needs the raw OpenImages patches behind get_nn_patches (out of scope, SURVEY.md §2 #8)")
    if opt.gpu < 0:
        raise SystemExit("rarm_sample.py (native): --gpu must name a HIP device; the native library has no CPU path")
    if opt.synthetic:
        model = LatentImageRETRO(transformer_config={"params": {}}, first_stage_config={"params": {"ddconfig": {}}}, k_nn=opt.k_nn, device=opt.gpu,
                                 nn_memory=np.arange(min(10_000, opt.synthetic_db_rows)))
        model.load_transformer_state_dict(synthetic.rarm_state_dict(model.rarm_cfg))
        fsd = synthetic.vq_state_dict(model.vq_cfg, synthetic.VQGAN_SEED)
        if opt.complete_from is not None or opt.score is not None:
            fsd.update(synthetic.vq_encoder_state_dict(model.vq_cfg))
        model.load_first_stage_state_dict(fsd)
        n = opt.synthetic_db_rows
        pool = {"embedding": synthetic.clip_like_rows(n), "img_id": np.arange(n), "patch_coords": np.zeros((n, 4), np.int64)}
        retr = ClipImageRetriever(state_dict=synthetic.clip_state_dict(_lib.make_clip_cfg()), ctx=model.ctx)
        model.retriever = DatasetBuilder(data_pool=pool, retriever=retr, ctx=model.ctx)
        return model.eval()
    import yaml
    model_dir = opt.model_path
    config_path, ckpt_path = model_dir / "config.yaml", model_dir / "model.ckpt"
    assert config_path.is_file(), f"Did not found config at {config_path}"
    assert ckpt_path.is_file(), f"Did not found ckpt at {ckpt_path}"
    cfg = yaml.safe_load(open(config_path))["model"]["params"]
    pl_sd = torch.load(ckpt_path, map_location="cpu")
    nn_memory, id_count = None, None
    if isinstance(cfg.get("nn_memory"), str) and os.path.isfile(cfg["nn_memory"]):
        import pickle
        with open(cfg["nn_memory"], "rb") as f:
            mem = pickle.load(f)
        nn_memory, id_count = mem["nn_memory"], mem.get("id_count")
    model = LatentImageRETRO(transformer_config=cfg["transformer_config"], first_stage_config=cfg["first_stage_config"],
                             mask_token=cfg.get("mask_token", 16384), sos_token=cfg.get("sos_token", 16385), nn_memory=nn_memory,
                             id_count=id_count, device=opt.gpu)
    model.load_state_dict(pl_sd["state_dict"])
    print("Loaded model.")
    if opt.clip_ckpt is None:
        raise SystemExit("rarm_sample.py (native): pass --clip_ckpt <ViT-B/32 state_dict>; the reference downloads it (no network here)")
    rp = dict(cfg["retrieval_cfg"]["params"])
    retr = ClipImageRetriever(state_dict=torch.load(opt.clip_ckpt, map_location="cpu"), ctx=model.ctx)
    model.retriever = DatasetBuilder(saved_embeddings=rp["saved_embeddings"], k=rp.get("k", 20), retriever=retr, ctx=model.ctx)
    return model.eval()


IMAGE_SUFFIXES = (".png", ".jpg", ".jpeg", ".bmp", ".webp")


def load_images(path, resolution, width=None):
    """Image file or directory (sorted) -> f32 [n,3,R,R] in [-1,1]: centre crop to a square, bicubic resize to the first-stage resolution.
    width: -> [n,3,resolution,width] instead, the centre crop taken at that aspect (rdm_sample.py --init_img at --height / --width)."""
    import torch
    from PIL import Image
    path = Path(path)
    files = sorted(f for f in path.iterdir() if f.suffix.lower() in IMAGE_SUFFIXES) if path.is_dir() else [path]
    if not files:
        raise SystemExit(f"no image found at {path}")
    out_h, out_w = resolution, (resolution if width is None else width)
    out = []
    for f in files:
        im = Image.open(f).convert("RGB")
        w, h = im.size
        cw, ch = (min(w, h), min(w, h)) if out_h == out_w else (min(w, h * out_w // out_h), min(h, w * out_h // out_w))
        left, top = (w - cw) // 2, (h - ch) // 2
        im = im.crop((left, top, left + cw, top + ch)).resize((out_w, out_h), Image.BICUBIC)
        out.append(torch.from_numpy(np.asarray(im, dtype=np.uint8).copy()).permute(2, 0, 1).float() / 127.5 - 1.0)
    return torch.stack(out)


def neighbours_of(model, opt, x):
    """The neighbour embeddings [bs,k,512] of an image batch: by its own CLIP embedding, or as -c / --only_caption / --unconditional say."""
    import torch
    from rdm_amd.modules.custom_clip.tokenizer import tokenize
    bs = x.shape[0]
    if opt.unconditional:
        return torch.zeros((bs, 1, 512), dtype=torch.float, device=model.device)
    if opt.caption != "":
        q = model.retriever.retriever.model.encode_text(torch.from_numpy(tokenize([opt.caption] * bs)))
    else:
        q = model.retriever.retriever(x)                     # the image's own CLIP embedding
    q = q.float()
    if opt.only_caption:
        assert opt.caption != "", "Need a caption"
        return q.unsqueeze(1).to(model.device)
    qe = q.cpu().numpy().astype(np.float32)
    nns, _ = model.retriever.searcher.search_batched(qe / np.linalg.norm(qe, axis=1)[:, np.newaxis], final_num_neighbors=opt.k_nn)
    return torch.from_numpy(np.asarray(model.retriever.data_pool["embedding"][nns])).to(model.device).to(torch.float)


def complete(model, opt):
    """[native] --complete_from: the `samples_half` / `reconstructions` entries of LatentImageRETRO.log_images (transformer.py:448-479) with
    a selectable split row, batch by batch over the given images."""
    import torch
    sampling_start = datetime.datetime.now().strftime("%Y-%m-%d-%H-%M-%S")
    cfg = model.vq_cfg
    side = cfg.resolution >> (cfg.n_ch_mult - 1)
    keep = side // 2 if opt.keep_rows is None else opt.keep_rows
    if not 0 <= keep < side:
        raise SystemExit(f"--keep_rows must lie in [0, {side}), got {keep}")
    images = load_images(opt.complete_from, cfg.resolution)
    if model.retriever is not None and model.retriever.searcher is None:
        model.train_searcher()
    for n in range(opt.n_runs):
        if opt.seed is not None:
            seed_everything(opt.seed)
        print(f"Run {n + 1}/{opt.n_runs}")
        for b0 in range(0, images.shape[0], opt.batch_size):
            x = images[b0:b0 + opt.batch_size].to(model.device)
            bs = x.shape[0]
            r = neighbours_of(model, opt, x)
            quant_z, z_indices = model.encode_to_z(x)
            _, c_indices = model.encode_to_c(torch.zeros((bs, 0)))
            z_start = z_indices[:, :keep * side]
            logs = {"samples_half": model.sampling_util(z_indices.shape[1] - z_start.shape[1], z_start, r, c_indices, opt.temperature, opt.top_k,
                                                        quant_z.shape, top_p=opt.top_p, guidance_scale=opt.guidance_scale,
                                                        prefill=opt.prefill),
                    "reconstructions": model.decode_to_img(z_indices, quant_z.shape)}
            for key, imgs in logs.items():
                for bi, be in enumerate(imgs):
                    save_image(be, os.path.join(opt.savepath, f"{sampling_start}-{key}-run{n}-sample{b0 + bi}.png"))
        if opt.increase_guidance:
            opt.guidance_scale += 1.0
            print(f"New guidance scale: {opt.guidance_scale}")
    print("Done")
    return sampling_start


def score(model, opt):
    """[native] --score: LatentImageRETRO.validation_step (transformer.py:65-70) image by image -> the per-token NLL tensor [n, codes]."""
    import torch
    images = load_images(opt.score, model.vq_cfg.resolution)
    if model.retriever is not None and model.retriever.searcher is None:
        model.train_searcher()
    if opt.seed is not None:
        seed_everything(opt.seed)
    rows = []
    for b0 in range(0, images.shape[0], opt.batch_size):
        x = images[b0:b0 + opt.batch_size].to(model.device)
        nll = model.nll(x, neighbours_of(model, opt, x)).cpu()
        for bi, row in enumerate(nll):
            m = float(row.mean())
            print(f"image {b0 + bi}: nll {m:.4f} nats/code, {m / np.log(2.0):.4f} bits/code")
        rows.append(nll)
    nll = torch.cat(rows)
    print(f"val/loss {float(nll.mean()):.4f}")
    return nll


def sample(model, opt):
    """rarm_sample.py:225-293."""
    if opt.score is not None:
        return score(model, opt)
    if getattr(opt, "complete_from", None) is not None:
        return complete(model, opt)
    import torch
    from rdm_amd.modules.custom_clip.tokenizer import tokenize
    qids = None
    sampling_start = datetime.datetime.now().strftime("%Y-%m-%d-%H-%M-%S")
    query_embeddings = None
    nn_embeddings = None
    if opt.caption != "":
        tokenized = torch.from_numpy(tokenize([opt.caption] * opt.batch_size))
        query_embeddings = model.retriever.retriever.model.encode_text(tokenized).cpu()
    if opt.only_caption:
        assert opt.caption != "", "Need a caption"
        nn_embeddings = query_embeddings.unsqueeze(1).to(model.device).float()
    elif opt.unconditional:
        nn_embeddings = torch.zeros((opt.batch_size, 1, 512), dtype=torch.float, device=model.device)
    for n in range(opt.n_runs):
        if opt.seed is not None:
            seed_everything(opt.seed)
        print("Sampling query and neighbors (wait for the sampling to start)")
        logs = model.sample_from_rdata(opt.batch_size, qids=qids, query_embeddings=query_embeddings, nn_embeddings=nn_embeddings,
                                       k_nn=opt.k_nn, return_nns=opt.save_nns, use_weights=opt.use_weights, memsize=opt.top_m,
                                       top_k=opt.top_k, temperature=opt.temperature, guidance_scale=opt.guidance_scale, top_p=opt.top_p)
        if opt.keep_qids:
            assert "qids" in logs
            qids = logs["qids"]
        print(f"Run {n + 1}/{opt.n_runs}")
        for key in logs:
            if key in ["samples_with_sampled_nns", "batched_nns"]:
                for bi, be in enumerate(logs[key]):
                    savename = os.path.join(opt.savepath, f'{sampling_start}-{key}-run{n}-sample{bi}.png')
                    if be.ndim == 3:
                        save_image(be, savename)
        if opt.increase_guidance:
            opt.guidance_scale += 1.0
            print(f"New guidance scale: {opt.guidance_scale}")
    print("Done")
    return sampling_start


if __name__ == "__main__":
    opt = parse_args()
    opt.savepath.mkdir(parents=True, exist_ok=True)
    model = load_model(opt)
    sample(model, opt)
