"""Native counterpart of the SAMPLING, VALIDATION and TRAINING methods of rdm/models/autoregression/transformer.py::LatentImageRETRO (RARM):
`forward` (:213-222), `shared_step` (:207-211), `get_mask_prob` (:186-189), `compute_loss` / `validation_step` (:46-48, :65-70: the
teacher-forced cross-entropy of an image's codes under its neighbours, one whole-sequence transformer pass), `sample` (:224-294), `sampling_util` (:296-312), `sample_from_rdata` (:314-404), `get_qids` (:407-430), `get_r` (:191-205),
`log_images` (:422-478: full samples, image completion from the first half of an image's codes, samples under masked neighbours,
reconstructions), and of the taming Net2NetTransformer pieces it inherits for them (`encode_to_z`, `encode_to_c` with the
SOSProvider, `decode_to_img`, `top_k_logits`).
`configure_optimizers` (:106-119) and `training_step` (:50-57) run one optimisation step on the native path (rdm_amd.training_rarm: the
transformer's forward with saved activations, the mean cross-entropy, the backward to every parameter, AdamW(betas=(0.9, 0.95)) on fp32
masters); `sync_sampling_weights` hands the trained weights to the sampling / validation kernels, `state_dict` returns them in the
reference's layout.  The LambdaLR scheduler of :109-118 and the Lightning loop stay with the caller (`training_step(..., lr=)`).
The patch plotter of log_images and image-patch neighbour encoders are out of scope (the shipped
configs use IdentityEncoder on CLIP embeddings, models/rarm/imagenet/dogs/config.yaml:10-13).

The transformer (rdm.modules.attention.RetrievalPatchTransformer, 18 x 768, causal self-attention + cross-attention to the k
retrieved neighbours), the VQGAN-f16 decoder and its encoder + nearest-code search run inside librdm_hip; the 256-step loop is ONE library call
(rdm_rarm_sample) that decodes against a K/V cache — the reference re-runs the whole prefix for every token (:241-248).
`prefill=True` (sample / sampling_util / log_images / sample_from_rdata) feeds a given prefix in one whole-sequence pass instead of token
by token (rdm_rarm_sample_prefill); the default stays the token-by-token feed.
The multinomial draw uses uniforms taken from torch's global generator on the model's device (so `seed_everything`
makes a run repeatable) and the inverse-CDF rule documented in include/rdm_hip.h.
"""
import numpy as np
import torch
import torch.nn.functional as F

from ... import _lib, packing, training_rarm


class LatentImageRETRO(object):
    def __init__(self, transformer_config, first_stage_config=None, mask_token=16384, sos_token=16385, nn_key="nn_embeddings",
                 nn_memory=None, id_count=None, retriever=None, k_nn=4, device=0, ctx=None, p_mask_max=0., **ignored):
        self._dev_index = device if isinstance(device, int) else (torch.device(device).index or 0)
        self._ctx = ctx
        self.device = getattr(ctx, "device", None) or torch.device("cuda", self._dev_index)
        tparams = transformer_config.get("params", transformer_config)
        self.rarm_cfg = _lib.make_rarm_cfg(**tparams)
        for flag, want in (("continuous", False), ("causal", True), ("cross_attend", True), ("positional_encodings", True)):
            if flag in tparams and bool(tparams[flag]) != want:
                raise NotImplementedError(f"RetrievalPatchTransformer with {flag}={tparams[flag]} (the shipped RARM configs use {want})")
        self.vq_cfg = None
        if first_stage_config is not None:
            fparams = first_stage_config.get("params", first_stage_config)
            dd = dict(fparams.get("ddconfig", {}))
            self.vq_cfg = _lib.make_vqgan_f16_cfg(embed_dim=fparams.get("embed_dim", 256), n_embed=fparams.get("n_embed", 16384),
                                                  z_channels=dd.get("z_channels", 256), ch=dd.get("ch", 128),
                                                  ch_mult=tuple(dd.get("ch_mult", (1, 1, 2, 2, 4))), num_res_blocks=dd.get("num_res_blocks", 2),
                                                  out_ch=dd.get("out_ch", 3), resolution=dd.get("resolution", 256),
                                                  attn_resolutions=tuple(dd.get("attn_resolutions", (16,))))
        self.sos_token, self.mask_token = int(sos_token), int(mask_token)
        self.nn_key, self.k_nn, self.p_mask_max = nn_key, k_nn, p_mask_max
        self.retriever = retriever
        self.nn_encoder = None                         # IdentityEncoder
        self.use_memory = nn_memory is not None
        if self.use_memory:
            self.nn_memory = torch.as_tensor(np.asarray(nn_memory))
        self.id_count = id_count
        self._transformer_sd = None                    # the state dict last loaded (a reference, not a copy): configure_optimizers' default
        self._train = None                             # (TrainState, shapes, optimiser settings) once configure_optimizers has run

    @property
    def ctx(self):
        if self._ctx is None:
            self._ctx = _lib.Context(self._dev_index)
        return self._ctx

    def eval(self): return self
    def to(self, device): return self

    # ---- weights: checkpoint keys `transformer.*` (RetrievalPatchTransformer) and `first_stage_model.*` (taming VQModel)
    def load_state_dict(self, sd, strict=True):
        tsd = packing.strip_prefix(sd, "transformer.") or sd
        self.load_transformer_state_dict(tsd)
        fsd = packing.strip_prefix(sd, "first_stage_model.")
        if fsd and self.vq_cfg is not None:
            self.load_first_stage_state_dict(fsd)
        return [], []

    def load_transformer_state_dict(self, tsd):
        self.ctx.load_rarm(self.rarm_cfg, packing.pack("rarm", self.rarm_cfg, tsd))
        self._transformer_sd = tsd

    def load_first_stage_state_dict(self, fsd):
        """Decoder + codebook always; the encoder (`encoder.*`, `quant_conv.*`: encode_to_z, log_images) when the dict carries it."""
        self.ctx.load_vq(self.vq_cfg, packing.pack("vq", self.vq_cfg, fsd))
        if any(k.startswith("encoder.") for k in fsd):
            self.ctx.load_vq_encoder(self.vq_cfg, packing.pack("vqenc", self.vq_cfg, fsd))

    # ---- taming pieces
    def encode_to_c(self, c):
        """cond_stage_config '__is_unconditional__' -> SOSProvider: one sos token per sample."""
        n = c.shape[0]
        idx = torch.full((n, 1), self.sos_token, dtype=torch.long)
        return idx, idx

    @torch.no_grad()
    def encode_to_z(self, x):
        """Net2NetTransformer.encode_to_z: image [b,3,R,R] in [-1,1] -> (quant_z [b,embed_dim,h,w], indices int64 [b, h*w])."""
        quant_z, indices = self.ctx.vq_encode_indices(x, return_quant=True)
        return quant_z, indices

    def get_xc(self, batch, N=None):
        """taming get_input on the `image` key ([N,H,W,3] -> [N,3,H,W] float); the conditioning is the SOS provider's: unused."""
        x = torch.as_tensor(batch["image"])
        if x.ndim == 3:
            x = x[..., None]
        x = x.permute(0, 3, 1, 2).to(dtype=torch.float32).contiguous()
        if N is not None:
            x = x[:N]
        return x, torch.zeros((x.shape[0], 0))

    # ---- transformer.py:191-205 (IdentityEncoder on [N,k,d] embeddings); the masking is host-side torch, as written there
    @torch.no_grad()
    def get_r(self, batch, N=None, p_mask=0.):
        nns = torch.as_tensor(batch[self.nn_key])
        if N is not None:
            nns = nns[:N]
        r = nns.to(torch.float32)
        if p_mask > 0.:
            mask = torch.bernoulli(torch.ones_like(r) * p_mask)
            mask = mask.round().to(dtype=torch.int64)
            r = r * (1 - mask) + mask * torch.ones_like(r) * self.mask_token
        return r

    @torch.no_grad()
    def decode_to_img(self, index, zshape=None):
        """Net2NetTransformer.decode_to_img: indices [b, h*w] -> image [b,3,256,256]."""
        return self.ctx.vq_decode_indices(index.reshape(index.shape[0], -1))

    def train_searcher(self):
        self.retriever.train_searcher()

    # ---- transformer.py:186-189, 207-222, 46-70: the teacher-forced pass (validation)
    def get_mask_prob(self):
        return np.random.uniform(0., self.p_mask_max)

    def _teacher_tokens(self, x, c):
        """-> (transformer input [cond | z][:, :-1], target z, cond length): :217-220"""
        _, z_indices = self.encode_to_z(x.to(self.device))
        _, cond = self.encode_to_c(c)
        cond = cond.to(z_indices.device)
        return torch.cat((cond, z_indices), 1)[:, :-1], z_indices, cond.shape[1]

    @torch.no_grad()
    def forward(self, x, c, r):
        """:213-222: logits of every code of x under the neighbours r (one whole-sequence pass) and the codes themselves."""
        tokens, target, nc = self._teacher_tokens(x, c)
        logits = self.ctx.rarm_forward_seq(tokens, r)
        return logits[:, nc - 1:], target

    __call__ = forward

    @torch.no_grad()
    def nll(self, x, r):
        """-log p(code) per token, f32 [b, h*w]: cross_entropy(reduction='none') of `forward`, without its [b, h*w, vocab] logits."""
        tokens, target, nc = self._teacher_tokens(x, torch.zeros((x.shape[0], 0)))
        assert nc == 1                                                      # the SOS provider: one conditioning token (encode_to_c)
        return self.ctx.rarm_nll(tokens, target, r)

    def shared_step(self, batch, batch_idx):
        x, c = self.get_xc(batch)
        r = self.get_r(batch, p_mask=self.get_mask_prob())
        return self.forward(x, c, r)

    def compute_loss(self, logits, targets, split="train"):
        loss = F.cross_entropy(logits.reshape(-1, logits.size(-1)), targets.reshape(-1))
        return loss, {f"{split}/loss": loss.detach()}

    @torch.no_grad()
    def validation_step(self, batch, batch_idx):
        """:65-70 -> {"val/loss": mean NLL}; through rdm_rarm_nll, so no [b, 256, 16384] logits tensor is formed."""
        x, c = self.get_xc(batch)
        r = self.get_r(batch, p_mask=self.get_mask_prob())
        return {"val/loss": self.nll(x, r).mean()}

    # ---- transformer.py:106-119, 50-57: the optimisation step (rdm_amd.training_rarm)
    def configure_optimizers(self, transformer_sd=None, lr=None, betas=(0.9, 0.95), eps=1e-8, weight_decay=1e-2):
        """:106-107: AdamW(self.transformer.parameters(), lr=self.learning_rate, betas=(0.9, 0.95)) with torch's eps and weight decay,
        on every transformer parameter.  Builds the train state -- fp32 masters and moments, bf16 working copies -- from `transformer_sd`
        (default: the state dict last loaded).  `lr` (default 1e-4) is what a step uses when it is not given one; the LambdaLR scheduler
        of :109-118 is the caller's."""
        sd = transformer_sd if transformer_sd is not None else self._transformer_sd
        if sd is None:
            raise RuntimeError("LatentImageRETRO.configure_optimizers: no transformer weights (load_state_dict / load_transformer_state_dict first, "
                               "or pass transformer_sd)")
        sd = packing.strip_prefix(sd, "transformer.") or sd
        shapes = {k: tuple(torch.as_tensor(v).shape) for k, v in sd.items()}
        state = training_rarm.TrainState(training_rarm.params_from_state_dict(sd, self.device))
        self._train = {"state": state, "shapes": shapes, "lr": 1e-4 if lr is None else float(lr), "betas": tuple(betas), "eps": float(eps),
                       "weight_decay": float(weight_decay)}
        return state

    def training_step(self, batch, batch_idx, lr=None):
        """:50-57 with the optimiser step of the training loop: shared_step's inputs (get_xc, encode_to_z, get_r under get_mask_prob()),
        the transformer input sos + codes[:, :-1], the mean cross-entropy, backward, AdamW.  -> the loss BEFORE the update (a float).
        The sampling / validation kernels keep the weights they were loaded with until sync_sampling_weights()."""
        if self._train is None:
            raise NotImplementedError("LatentImageRETRO.training_step: the native backward pass is set up by configure_optimizers() -- call it "
                                      "first (validation_step, nll and forward need no set-up)")
        x, c = self.get_xc(batch)
        r = self.get_r(batch, p_mask=self.get_mask_prob())
        tokens, target, nc = self._teacher_tokens(x, c)
        assert nc == 1                                                      # the SOS provider: one conditioning token (encode_to_c)
        tr = self._train
        return training_rarm.rarm_training_step(self.ctx, tr["state"], self.rarm_cfg, tokens, target, r, lr=tr["lr"] if lr is None else float(lr),
                                                betas=tr["betas"], eps=tr["eps"], weight_decay=tr["weight_decay"])

    def state_dict(self):
        """The trained `transformer.*` tensors in the reference's layout (host fp32); before configure_optimizers: the loaded ones."""
        if self._train is None:
            if self._transformer_sd is None:
                raise RuntimeError("LatentImageRETRO.state_dict: no transformer weights loaded")
            return {"transformer." + k: torch.as_tensor(v) for k, v in self._transformer_sd.items()}
        sd = training_rarm.state_dict_from_params(self._train["state"].P, self._train["shapes"])
        return {"transformer." + k: v for k, v in sd.items()}

    def sync_sampling_weights(self):
        """Re-pack the live (trained) weights and load them into the library: validation_step, nll, forward and sample see the trained model."""
        if self._train is None:
            raise RuntimeError("LatentImageRETRO.sync_sampling_weights: configure_optimizers() has not run")
        tsd = training_rarm.state_dict_from_params(self._train["state"].P, self._train["shapes"])
        self.ctx.load_rarm(self.rarm_cfg, packing.pack("rarm", self.rarm_cfg, tsd))
        self._transformer_sd = tsd

    # ---- transformer.py:224-294
    @torch.no_grad()
    def sample(self, x, r, c, steps, temperature=1.0, sample=False, top_k=None, guidance_scale=1.0, callback=lambda k: None,
               uniforms=None, top_p=None, prefill=None, **kwargs):
        """`top_p` (:279-280 names it and asserts it away): the nucleus filter after top-k, in (0, 1]; None and 1.0 are the call
        without one.  With sample=False (arg-max) it has no effect, as top_k has none.
        `prefill`: feed [c | x] in one whole-sequence pass (rdm_rarm_sample_prefill) instead of token by token; None / False: token by token."""
        top_p = _lib.check_top_p("LatentImageRETRO.sample", top_p)
        x = torch.cat((c.to(self.device), x.to(self.device)), 1)           # conditioning tokens, then any given prefix
        for k_ in range(steps):
            callback(k_)                                                    # the loop itself runs inside the library
        if uniforms is None:
            uniforms = torch.rand((steps, x.shape[0]), device=self.device)
        if not sample:
            top_k, top_p = 1, None                                          # torch.topk(probs, 1): the arg-max token (:266-267)
        extra = {}
        if top_p is not None:
            extra["top_p"] = top_p
        if prefill:
            extra["prefill"] = True
        new = self.ctx.rarm_sample(x, r, steps, uniforms, temperature=temperature, top_k=top_k, guidance_scale=guidance_scale, **extra)
        if x.shape[1] == c.shape[1]:
            return new
        return torch.cat((x[:, c.shape[1]:].to(torch.int64), new), 1)      # the given prefix, then the new tokens (:268-269)

    # ---- transformer.py:296-312
    @torch.no_grad()
    def sampling_util(self, steps, z_start, r, c, temperature, top_k, zshape, callback=None, top_p=1., **kwargs):
        index_sample = self.sample(z_start, r, c, steps=steps, temperature=temperature if temperature is not None else 1.0,
                                   sample=True, top_k=top_k if top_k is not None else 100, top_p=top_p,
                                   callback=callback if callback is not None else lambda k: None, **kwargs)
        return self.decode_to_img(index_sample, zshape)

    # ---- transformer.py:314-404 (IdentityEncoder branch; return_nns needs the raw patches: out of scope)
    @torch.no_grad()
    def sample_from_rdata(self, N, cond=None, return_nns=False, use_weights=False, qids=None, k_nn=None, memsize=100, verbose=False,
                          top_k=256, temperature=1.0, code_side_len=16, z_dimensionality=256, pre_loaded_patches=None,
                          nn_embeddings=None, query_embeddings=None, top_p=None, db_subset=None, **kwargs):
        """db_subset [native]: the neighbours come from a named subset of the database (retriever.define_subset), a name or one name (or
        None) per sample; the pseudo-queries are drawn as before."""
        if return_nns or pre_loaded_patches is not None:
            raise NotImplementedError("return_nns / pre_loaded_patches need the raw OpenImages patches (out of scope, SURVEY.md §2 #8)")
        if cond is not None:
            raise NotImplementedError()
        if self.retriever is not None and self.retriever.searcher is None:
            self.train_searcher()
        if k_nn is None:
            k_nn = self.k_nn
        out = {}
        if nn_embeddings is None:
            if query_embeddings is None:
                qids = self.get_qids(memsize, N, qids=qids, use_weights=use_weights, verbose=verbose)
                out["qids"] = qids
                query_embeddings = self.retriever.data_pool['embedding'][qids]
            qe = query_embeddings.cpu().numpy() if isinstance(query_embeddings, torch.Tensor) else np.asarray(query_embeddings)
            qe = qe.astype(np.float32)
            nns, _ = self.retriever.search_subset(qe / np.linalg.norm(qe, axis=1)[:, np.newaxis], k_nn, db_subset)
            retro_cond = torch.from_numpy(np.asarray(self.retriever.data_pool['embedding'][nns])).to(self.device).to(torch.float)
        else:
            retro_cond = nn_embeddings
        _, cond = self.encode_to_c(torch.zeros((N, 0)))
        z_shape = (N, z_dimensionality, code_side_len, code_side_len)
        steps = code_side_len ** 2
        z_start = torch.zeros((N, 0), dtype=torch.long)
        out["samples_with_sampled_nns"] = self.sampling_util(steps, z_start, retro_cond, cond, temperature, top_k, z_shape, top_p=top_p, **kwargs)
        return out

    # ---- transformer.py:422-478.  plot_cond_stage is a no-op for the SOS provider; the patch plotter needs the raw patches (out of scope)
    @torch.no_grad()
    def log_images(self, batch, temperature=None, top_k=256, top_p=1.0, callback=None, N=4, half_sample=True, sample=True, p_sample=True,
                   masking_probs=[0.5, 1.0], **kwargs):
        log = dict()
        x, c = self.get_xc(batch, N)
        r = self.get_r(batch, N, p_mask=0.)
        x = x.to(device=self.device)
        r = r.to(device=self.device)
        quant_z, z_indices = self.encode_to_z(x)
        _, c_indices = self.encode_to_c(c)
        n = z_indices.shape[1]
        if sample:
            log["samples_full"] = self.sampling_util(n, z_indices[:, :0], r, c_indices, zshape=quant_z.shape, temperature=temperature,
                                                     top_k=top_k, top_p=top_p, callback=callback, **kwargs)
        if half_sample:
            z_start_indices = z_indices[:, :n // 2]
            log["samples_half"] = self.sampling_util(n - z_start_indices.shape[1], z_start_indices, r, c_indices, temperature=temperature,
                                                     top_k=top_k, top_p=top_p, callback=callback, zshape=quant_z.shape, **kwargs)
        if p_sample:
            if masking_probs[0] >= self.p_mask_max and self.p_mask_max != 0.:
                masking_probs = [self.p_mask_max] + masking_probs
            for p_mask in masking_probs:
                r = self.get_r(batch, N, p_mask=p_mask).to(device=self.device)
                log[f"samples_full_p_{p_mask:.2f}"] = self.sampling_util(n, z_indices[:, :0], r, c_indices, zshape=quant_z.shape,
                                                                         temperature=temperature, top_k=top_k, top_p=top_p, callback=callback, **kwargs)
        log["inputs"] = x
        log["reconstructions"] = self.decode_to_img(z_indices, quant_z.shape)
        return log

    # ---- transformer.py:407-430
    def get_qids(self, memsize, N, qids=None, use_weights=False, verbose=False):
        if isinstance(memsize, float):
            assert memsize > 0 and memsize <= 1., 'Require memsize in (0,1]'
            memsize = int(memsize * self.nn_memory.shape[0])
        if qids is None:
            if self.use_memory:
                memsize = min(memsize, self.nn_memory.shape[0])
                nn_mem = self.nn_memory.detach().cpu().numpy()[:memsize]
                ps = None
                if use_weights:
                    freqs = np.asarray([self.id_count[int(id_)] for id_ in nn_mem])
                    ps = freqs / freqs.sum(keepdims=True)
                qids = np.random.choice(nn_mem, size=N, p=ps)
            else:
                qids = np.random.choice(len(self.retriever.data_pool['embedding']), size=N)
        else:
            assert qids.shape[0] == N
        return qids
