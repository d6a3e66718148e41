"""rdm/util.py counterparts used on the sampling path."""
import numpy as np
import torch


def ischannellastimage(x) -> bool:
    """rdm/util.py:17-20."""
    return hasattr(x, "shape") and len(x.shape) == 4 and x.shape[-1] in (1, 3)


def convert_nn_tree(nn_tree):
    """rdm/util.py:23-30: ScaNN ids uint32 -> int32 (recursively over dict / array)."""
    if isinstance(nn_tree, dict):
        return {k: convert_nn_tree(v) for k, v in nn_tree.items()}
    if isinstance(nn_tree, np.ndarray) and nn_tree.dtype == np.uint32:
        return nn_tree.astype(np.int32)
    return nn_tree


def instantiate_from_config(config):
    """ldm.util.instantiate_from_config for `target:` / `params:` trees, with rdm.* / ldm.* targets that have a
    native counterpart redirected to rdm_amd.*"""
    import importlib
    target = config["target"]
    redirect = {
        "rdm.models.diffusion.ddpm.MinimalRETRODiffusion": "rdm_amd.models.diffusion.ddpm.MinimalRETRODiffusion",
        "rdm.data.retrieval_dataset.dsetbuilder.DatasetBuilder": "rdm_amd.data.retrieval_dataset.dsetbuilder.DatasetBuilder",
        "rdm.modules.retrievers.ClipImageRetriever": "rdm_amd.modules.retrievers.ClipImageRetriever",
        "rdm.modules.retrievers.CLIPTextEmbedder": "rdm_amd.modules.retrievers.CLIPTextEmbedder",
        "rdm.models.autoregression.transformer.LatentImageRETRO": "rdm_amd.models.autoregression.transformer.LatentImageRETRO",
    }
    target = redirect.get(target, target)
    mod, cls = target.rsplit(".", 1)
    return getattr(importlib.import_module(mod), cls)(**config.get("params", dict()))


# ---- [native] the neighbour bias of the UNet's cross-attention (include/rdm_hip.h rdm_set_neighbour_bias), formed on the host
def check_neighbour_bias(bias, rows=None, k=None):
    """A caller's bias as the library takes it: fp32 [rows, k], finite values or -inf, every row with a finite entry -> the CPU tensor.
    The library checks the same (a refused bias there is an RdmError); this is the ValueError of the Python surface, before any GPU work."""
    b = torch.as_tensor(bias).detach().to("cpu", torch.float32)
    if b.ndim != 2 or (rows is not None and b.shape[0] != rows) or (k is not None and b.shape[1] != k):
        raise ValueError(f"neighbour_bias must be [{'B' if rows is None else rows}, {'k' if k is None else k}], got {tuple(b.shape)}")
    if bool(torch.isnan(b).any()):
        raise ValueError("neighbour_bias holds NaN")
    if bool((b == float("inf")).any()):
        raise ValueError("neighbour_bias holds +inf (finite values and -inf only)")
    dead = (~torch.isfinite(b)).all(dim=1).nonzero()
    if dead.numel():
        raise ValueError(f"neighbour_bias row {int(dead[0])} has no finite entry: a sample must keep at least one neighbour")
    return b.contiguous()


def neighbour_bias_from(n, k, nn_counts=None, nn_weights=None, n_reps=None):
    """nn_counts / nn_weights of sample_with_query / sample_from_rdata -> the bias [n, k (* n_reps)] or None when neither is given.
    nn_counts: an int, or one per sample, in [1, k]: sample b attends the first nn_counts[b] entries of its conditioning (-inf on the
    rest).  nn_weights: [n, k] (or [k], for every sample), non-negative and finite: entry j counts w times (bias log w; 0 = absent).
    Both: the sum.  n_reps: the conditioning is tiled n_reps times along the neighbour axis, and so is the bias."""
    if nn_counts is None and nn_weights is None:
        return None
    bias = torch.zeros(n, k)
    if nn_counts is not None:
        c = np.asarray(nn_counts)
        if c.ndim == 0:
            c = np.full((n,), c)
        if c.shape != (n,) or not np.issubdtype(c.dtype, np.integer):
            raise ValueError(f"nn_counts must be an int or {n} ints (one per sample), got {nn_counts!r}")
        if c.min() < 1 or c.max() > k:
            raise ValueError(f"nn_counts must lie in [1, {k}] (k_nn), got values in [{c.min()}, {c.max()}]")
        bias = bias.masked_fill(torch.arange(k)[None, :] >= torch.from_numpy(c.astype(np.int64))[:, None], float("-inf"))
    if nn_weights is not None:
        w = torch.as_tensor(nn_weights).detach().to("cpu", torch.float64)
        if w.ndim == 1:
            w = w[None].expand(n, -1)
        if tuple(w.shape) != (n, k):
            raise ValueError(f"nn_weights must be [{n}, {k}] (or [{k}]), got {tuple(torch.as_tensor(nn_weights).shape)}")
        if not bool(torch.isfinite(w).all()) or bool((w < 0).any()):
            raise ValueError("nn_weights must be finite and non-negative (0 = the neighbour is absent)")
        bias = bias + torch.log(w).float()           # log 0 = -inf
    bias = check_neighbour_bias(bias, n, k)
    if n_reps is not None:
        bias = torch.cat([bias] * int(n_reps), dim=1)
    return bias.contiguous()


def takes_neighbour_bias(ctx_of):
    """Decorator of a sampling method: it accepts neighbour_bias= ([B, k], see check_neighbour_bias), sets it on the native context
    ctx_of(self) around the call -- the native loop, or every forward of a per-step path -- and clears it on the way out."""
    import functools

    def deco(fn):
        @functools.wraps(fn)
        def wrapped(self, *args, neighbour_bias=None, **kwargs):
            if neighbour_bias is None:
                return fn(self, *args, **kwargs)
            with ctx_of(self).neighbour_bias(check_neighbour_bias(neighbour_bias)):
                return fn(self, *args, **kwargs)
        return wrapped
    return deco
