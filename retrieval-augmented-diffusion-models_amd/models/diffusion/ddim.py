"""SAMPLING ONLY — native counterpart of rdm/models/diffusion/ddim.py:14-268 (DDIMSampler).

Same constructor, `make_schedule`, `sample`, `ddim_sampling`, `p_sample_ddim` signatures and return values; the
S-step loop itself runs inside librdm_hip (rdm_ddim_sample): UNet forward with CFG batch doubling + fused update
per step, K/V of the neighbours projected once per call.  Options that change the loop body per step (callbacks, mask / x0
inpainting, style_cond / content_cond by SNR band, timestep subset, noise_dropout, score_corrector) take the per-step path:
native UNet forward, torch elementwise update.  quantize_x0 (round 4) also takes the per-step path: pred_x0 is snapped to the
first stage's codebook by the native quantiser (rdm_vq_quantize).  ddim_use_original_steps raises NotImplementedError: in the
reference that branch reads `self.model.ddim_sigmas_for_original_num_steps` (ddim.py:249), a buffer make_schedule registers on the
SAMPLER (:52), so it ends in AttributeError there -- dead code, not a feature to mirror.  Unlike the reference, nothing is forced
onto a "cuda" device string (ddim.py:21-25) and `--seed` style RNG comes from the caller's torch generator.

Image-to-image -- `stochastic_encode`, `encode`, `decode`, which ldm's DDIMSampler has and the reference's vendored copy stops before -- is
added on ldm's surface at the end of the class: the noised start, deterministic DDIM inversion and the partial decode, each a native
loop or kernel (rdm_op_q_sample_seeded, rdm_ddim_encode, rdm_ddim_decode) with a per-step path behind `callback`.
"""
import contextlib

import numpy as np
import torch

from ...util import takes_neighbour_bias

_biased = takes_neighbour_bias(lambda sampler: sampler.model.ctx)      # sample / decode / encode(..., neighbour_bias=[B, k])


def make_ddim_timesteps(ddim_discr_method, num_ddim_timesteps, num_ddpm_timesteps, verbose=True):
    if ddim_discr_method != "uniform":
        raise NotImplementedError(f'ddim discretization "{ddim_discr_method}"')
    c = num_ddpm_timesteps // num_ddim_timesteps
    ts = np.asarray(list(range(0, num_ddpm_timesteps, c))) + 1      # NB: S that does not divide T yields > S steps (ldm quirk)
    if ts[-1] >= num_ddpm_timesteps:
        raise ValueError(f"S={num_ddim_timesteps} gives ddim timestep {ts[-1]} >= T={num_ddpm_timesteps} "
                         "(the reference indexes alphas_cumprod out of range for this S)")
    return ts


def make_ddim_sampling_parameters(alphacums, ddim_timesteps, eta, verbose=True):
    a = np.asarray(alphacums, dtype=np.float32)
    alphas = a[ddim_timesteps]
    alphas_prev = np.asarray([a[0]] + a[ddim_timesteps[:-1]].tolist())          # float64 array of fp32 values
    sigmas = eta * np.sqrt((1 - alphas_prev) / (1 - alphas) * (1 - alphas / alphas_prev))
    return sigmas, alphas, alphas_prev


class _SamplerBase(object):
    """What DDIMSampler, PLMSSampler, DPMSolverSampler and UniPCSampler share: the constructor, DDIM's schedule, the guided model output
    of the per-step paths, and the rules the loops apply around a step."""

    def __init__(self, model, schedule="linear", **kwargs):
        super().__init__()
        self.model = model
        self.ddpm_num_timesteps = model.num_timesteps
        self.schedule = schedule

    def register_buffer(self, name, attr):
        setattr(self, name, attr)

    def make_schedule(self, ddim_num_steps, ddim_discretize="uniform", ddim_eta=0., verbose=True):
        self.ddim_timesteps = make_ddim_timesteps(ddim_discretize, ddim_num_steps, self.ddpm_num_timesteps, verbose)
        self.ddim_num_steps, self.ddim_eta = int(ddim_num_steps), float(ddim_eta)      # what encode / decode hand to the native loops
        ac = self.model.alphas_cumprod.detach().float().cpu()
        assert ac.shape[0] == self.ddpm_num_timesteps, 'alphas have to be defined for each timestep'
        self.register_buffer('alphas_cumprod', ac)
        sig, al, alp = make_ddim_sampling_parameters(ac.numpy(), self.ddim_timesteps, ddim_eta, verbose)
        self.register_buffer('ddim_sigmas', sig)
        self.register_buffer('ddim_alphas', al)
        self.register_buffer('ddim_alphas_prev', alp)
        self.register_buffer('ddim_sqrt_one_minus_alphas', np.sqrt(1. - al))

    @staticmethod
    def _unwrap(c, single=None):
        """A conditioning given as a dict (its first value) or a list (its first entry).  `single` names the loop that takes one
        cross-attention tensor only and refuses a longer list."""
        if isinstance(c, dict):
            c = c[list(c.keys())[0]]
        if isinstance(c, (list, tuple)):
            if single is not None and len(c) != 1:
                raise NotImplementedError(f"native {single} loop takes a single cross-attention conditioning tensor")
            c = c[0]
        return c

    @staticmethod
    def _refuse_original_steps(ddim_use_original_steps):
        if ddim_use_original_steps:
            raise NotImplementedError("ddim_use_original_steps: dead in the reference (ddim.py:249 reads a buffer that lives on the sampler, "
                                      "not on the model: AttributeError)")

    @staticmethod
    def _one_noise_source(noise_seed, noise, noun="noise stack"):
        """[native] A noise_seed selects the library's generator, an explicit `noise` the caller's values: never both."""
        if noise_seed is not None and noise is not None:
            raise ValueError(f"noise_seed and an explicit {noun} select different noise sources: give one of them")

    def _timestep_subset(self, timesteps):
        if timesteps is None:
            return self.ddim_timesteps
        subset_end = int(min(timesteps / self.ddim_timesteps.shape[0], 1) * self.ddim_timesteps.shape[0]) - 1     # ddim.py:158-160
        return self.ddim_timesteps[:subset_end]

    @staticmethod
    def _logs(index, log_every_t, total_steps):
        return index % log_every_t == 0 or index == total_steps - 1

    @staticmethod
    def _warn_batch(conditioning, batch_size):
        if conditioning is not None and not isinstance(conditioning, (dict, list)):
            if conditioning.shape[0] != batch_size:
                print(f"Warning: Got {conditioning.shape[0]} conditionings but batch-size is {batch_size}")

    @staticmethod
    def _intermediates(img, x_inter, pred_x0, to_cpu=False):
        """The start latent, then what a native loop logged."""
        mv = (lambda t: t.detach().cpu()) if to_cpu else (lambda t: t)
        return {'x_inter': [img] + [mv(t) for t in x_inter], 'pred_x0': [img] + [mv(t) for t in pred_x0]}

    def _device_randn(self, size, noise_seed, noise_row0=0, step=0, stream=0):
        """[native] The library's own normals (Context.op_randn: a function of (seed, stream, step, global row, element) only) at the
        latent size (B, C, H, W), rows noise_row0 .. noise_row0 + B - 1: stream 0 / step 0 is the starting latent of a seeded sampling
        call, stream 1 / step i the update noise of loop step i."""
        size = tuple(int(v) for v in size)
        return self.model.ctx.op_randn(noise_seed, size[0], int(np.prod(size[1:])), row0=noise_row0, step=step, stream=stream).reshape(size)

    def _seeded_start(self, x_T, size, noise_seed, noise_row0=0):
        """x_T when given; else, with a noise_seed, the library's starting latent (stream 0); else None (the caller draws with torch)."""
        if x_T is not None or noise_seed is None:
            return x_T
        return self._device_randn(size, noise_seed, noise_row0)

    def _model_output(self, x, t, c, uc, scale, score_corrector=None, corrector_kwargs=None, uncond_first=False):
        """eps of the per-step paths: one forward, or (uc given and scale != 1) one forward of the doubled batch [c | uc] -- ldm's PLMS
        order [uc | c] with uncond_first: the library's zero-context shortcut keys on TRAILING all-zero rows -- combined as
        e_u + scale (e_c - e_u); then the score corrector."""
        if uc is None or scale == 1.:
            e_t = self.model.apply_model(x, t, c)
        else:
            b = x.shape[0]
            ctx = getattr(self.model, "ctx", None)      # a neighbour bias in force belongs to the b conditional rows of the doubled batch
            with (ctx.neighbour_bias_doubled(uncond_first) if hasattr(ctx, "neighbour_bias_doubled") else contextlib.nullcontext()):
                out = self.model.apply_model(torch.cat([x] * 2), torch.cat([t] * 2), torch.cat([uc, c] if uncond_first else [c, uc]))
            e_c, e_u = (out[b:], out[:b]) if uncond_first else (out[:b], out[b:])
            e_t = e_u + scale * (e_c - e_u)
        if score_corrector is not None:
            assert getattr(self.model, "parameterization", "eps") == "eps"
            e_t = score_corrector.modify_score(self.model, e_t, x, t, c, **(corrector_kwargs or {}))
        return e_t

    def _masked_blend(self, img, mask, x0, ts, q_noise):
        """Inpainting: outside the mask keep the sample, inside take x0 noised to the step's timestep."""
        assert x0 is not None
        img_orig = self._q_sample(x0, ts, q_noise)
        return img_orig * mask + (1. - mask) * img

    def _q_sample(self, x_start, t, noise=None):
        """The model's q_sample; a model without one (a stand-in) gets it restated from its alphas_cumprod."""
        if hasattr(self.model, "q_sample"):
            return self.model.q_sample(x_start, t, noise=noise)
        noise = torch.randn_like(x_start) if noise is None else noise
        ac = self.model.alphas_cumprod.detach().double().cpu()
        sa = torch.sqrt(ac).float().to(x_start.device)[t].reshape(-1, 1, 1, 1)
        s1m = torch.sqrt(1. - ac).float().to(x_start.device)[t].reshape(-1, 1, 1, 1)
        return sa * x_start + s1m * noise


class DDIMSampler(_SamplerBase):

    @_biased
    @torch.no_grad()
    def sample(self, S, batch_size, shape, conditioning=None, callback=None, normals_sequence=None, img_callback=None,
               quantize_x0=False, eta=0., mask=None, x0=None, temperature=1., noise_dropout=0., score_corrector=None,
               corrector_kwargs=None, verbose=True, x_T=None, log_every_t=100, unconditional_guidance_scale=1.,
               unconditional_conditioning=None, random_guiding='none', r_shape=None, retro_cond=None,
               return_neighbors=False, k_nn=None, ignore_noising=False, content_cond=None, style_cond=None,
               intermediates_to_cpu=False, noise_seed=None, noise_row0=0, **kwargs):
        """`noise_seed` / `noise_row0` [native]: take the starting latent (when no x_T is given) and the per-step noise of eta > 0 from
        the library's counter-based generator, rows noise_row0 .. noise_row0 + batch_size - 1 of that seed: no noise stack exists, and a
        row's sample does not depend on how a batch is sharded.  Default None: torch's generator, as before."""
        self._warn_batch(conditioning, batch_size)
        self.make_schedule(ddim_num_steps=S, ddim_eta=eta, verbose=verbose)
        size = (batch_size,) + tuple(shape)
        return self.ddim_sampling(conditioning, size, callback=callback, img_callback=img_callback,
                                  quantize_denoised=quantize_x0, mask=mask, x0=x0, noise_dropout=noise_dropout,
                                  temperature=temperature, score_corrector=score_corrector, corrector_kwargs=corrector_kwargs, x_T=x_T,
                                  log_every_t=log_every_t, unconditional_guidance_scale=unconditional_guidance_scale,
                                  unconditional_conditioning=unconditional_conditioning, random_guiding=random_guiding,
                                  content_cond=content_cond, style_cond=style_cond,
                                  intermediates_to_cpu=intermediates_to_cpu, S=S, eta=eta, noise=kwargs.get("noise"),
                                  q_noise=kwargs.get("q_noise"), noise_seed=noise_seed, noise_row0=noise_row0)

    @torch.no_grad()
    def ddim_sampling(self, cond, shape, x_T=None, ddim_use_original_steps=False, callback=None, timesteps=None,
                      quantize_denoised=False, mask=None, x0=None, img_callback=None, log_every_t=100, temperature=1.,
                      noise_dropout=0., score_corrector=None, corrector_kwargs=None, unconditional_guidance_scale=1.,
                      unconditional_conditioning=None, random_guiding='none', content_cond=None, style_cond=None,
                      intermediates_to_cpu=False, S=None, eta=0., noise_seed=None, noise_row0=0, **kwargs):
        self._refuse_original_steps(ddim_use_original_steps)
        self._one_noise_source(noise_seed, kwargs.get("noise"))
        # options that change the loop body step by step run through the per-step path (native UNet forward per step)
        per_step = (quantize_denoised or mask is not None or x0 is not None or noise_dropout > 0. or score_corrector is not None or
                    content_cond is not None or style_cond is not None or random_guiding != 'none' or timesteps is not None)
        cond = self._unwrap(cond, single="DDIM")
        unconditional_conditioning = self._unwrap(unconditional_conditioning)
        assert unconditional_guidance_scale >= 1.
        if unconditional_guidance_scale > 1.:
            assert unconditional_conditioning is not None
        device = self.model.device
        x_T = self._seeded_start(x_T, shape, noise_seed, noise_row0)
        img = torch.randn(shape, device=device) if x_T is None else x_T.to(device)
        total_steps = self.ddim_timesteps.shape[0]
        print(f"Running DDIM Sampling with {total_steps} timesteps")
        if callback is not None or img_callback is not None or per_step:
            return self._python_loop(cond, img, callback, img_callback, log_every_t, temperature, eta,
                                     unconditional_guidance_scale, unconditional_conditioning, intermediates_to_cpu,
                                     mask=mask, x0=x0, noise_dropout=noise_dropout, score_corrector=score_corrector,
                                     corrector_kwargs=corrector_kwargs, random_guiding=random_guiding, timesteps=timesteps,
                                     content_cond=self._unwrap(content_cond), style_cond=self._unwrap(style_cond),
                                     noise=kwargs.get("noise"), q_noise=kwargs.get("q_noise"), quantize_denoised=quantize_denoised,
                                     noise_seed=noise_seed, noise_row0=noise_row0)
        noise = kwargs.get("noise")             # [native] optional explicit per-step noise stack [S, B, C, H, W] (consumed in loop order)
        seeded = {} if noise_seed is None else dict(seed=noise_seed, row0=noise_row0)      # [native] the step kernel generates the noise
        if eta != 0. and noise is None and noise_seed is None:
            noise = torch.randn((total_steps,) + tuple(shape), device=device)
        z, xi, pi = self.model.ctx.ddim_sample(S, img, cond, unconditional_conditioning if unconditional_guidance_scale > 1. else None,
                                               self.alphas_cumprod, eta=eta, scale=unconditional_guidance_scale, noise=noise,
                                               log_every_t=log_every_t, temperature=temperature, want_intermediates=True, **seeded)
        return z.detach(), self._intermediates(img, xi, pi, intermediates_to_cpu)

    def _python_loop(self, cond, img, callback, img_callback, log_every_t, temperature, eta, scale, uc, to_cpu, mask=None,
                     x0=None, noise_dropout=0., score_corrector=None, corrector_kwargs=None, random_guiding='none',
                     timesteps=None, content_cond=None, style_cond=None, noise=None, q_noise=None, quantize_denoised=False,
                     noise_seed=None, noise_row0=0, ts_all=None, q_noise_seed=None):
        """Per-step path of ddim.py:143-209 (callbacks, inpainting mask, style / content conditioning by SNR band, timestep
        subset, noise dropout, score corrector): native UNet forward per step, torch elementwise update.  `noise` / `q_noise`
        [native]: optional explicit stacks [steps, B, C, H, W] for the update noise and for q_sample of the masked region;
        `noise_seed` [native]: step i's update noise is the library's (stream 1, step i), what the native seeded loop applies.
        `ts_all` [native]: the ascending timesteps to run down (decode: the schedule's first t_start) instead of `timesteps`' subset.
        `q_noise_seed` [native]: without a q_noise stack, step i's q_sample noise is the library's (stream 0, step i + 1) of that seed, rows
        noise_row0 .. -- what the native seeded inpainting loop applies (decode passes its noise_seed); None: torch's generator, which is
        what sample(mask=, noise_seed=) keeps drawing it from."""
        if ts_all is None:
            ts_all = self._timestep_subset(timesteps)
        total_steps = ts_all.shape[0]
        intermediates = {'x_inter': [img], 'pred_x0': [img]}
        b = img.shape[0]
        random_guider = None
        if random_guiding != 'none':                                # drawn (RNG parity) but unused, as in the reference (:228)
            random_guider = torch.clamp(torch.randn(img.shape, device=img.device), -1., 1.)
        for i, step in enumerate(np.flip(ts_all)):
            index = total_steps - i - 1
            ts = torch.full((b,), int(step), device=img.device, dtype=torch.long)
            snr = self.ddim_alphas[index] / (1 - self.ddim_alphas[index])
            input_cond = cond
            if style_cond is not None and snr < 5.e-2:
                input_cond = style_cond
            if content_cond is not None and snr >= 5.e-2 and snr < 1.:
                input_cond = content_cond
            if mask is not None:
                qn = (q_noise[i] if q_noise is not None else None if q_noise_seed is None else
                      self._device_randn(img.shape, q_noise_seed, noise_row0, step=i + 1, stream=0))
                img = self._masked_blend(img, mask, x0, ts, qn)
            if random_guiding == 'sampled':
                random_guider = torch.clamp(torch.randn(img.shape, device=img.device), -1., 1.)
            img, pred_x0 = self.p_sample_ddim(img, input_cond, ts, index=index, temperature=temperature, quantize_denoised=quantize_denoised,
                                              noise_dropout=noise_dropout, score_corrector=score_corrector,
                                              corrector_kwargs=corrector_kwargs, unconditional_guidance_scale=scale,
                                              unconditional_conditioning=uc,
                                              noise=(noise[i] if noise is not None else None if noise_seed is None or eta == 0. else
                                                     self._device_randn(img.shape, noise_seed, noise_row0, step=i, stream=1)),
                                              random_guider=random_guider)
            if callback: callback(i)
            if img_callback: img_callback(pred_x0, i)
            if self._logs(index, log_every_t, total_steps):
                intermediates['x_inter'].append(img.cpu() if to_cpu else img)
                intermediates['pred_x0'].append(pred_x0.cpu() if to_cpu else pred_x0)
        return img, intermediates

    @torch.no_grad()
    def p_sample_ddim(self, x, c, t, index, use_original_steps=False, quantize_denoised=False, temperature=1.,
                      noise_dropout=0., score_corrector=None, corrector_kwargs=None, unconditional_guidance_scale=1.,
                      unconditional_conditioning=None, noise=None, random_guider=None):
        assert unconditional_guidance_scale >= 1.
        if use_original_steps:
            raise NotImplementedError("use_original_steps: dead in the reference (ddim.py:249)")
        if noise is None:
            noise = torch.randn(x.shape, device=x.device)
        if unconditional_guidance_scale > 1.:
            assert unconditional_conditioning is not None
        e_t = self._model_output(x, t, c, unconditional_conditioning if unconditional_guidance_scale > 1. else None,
                                 unconditional_guidance_scale, score_corrector, corrector_kwargs)
        a_t = torch.full_like(e_t, float(self.ddim_alphas[index]))
        a_prev = torch.full_like(e_t, float(self.ddim_alphas_prev[index]))
        sigma_t = torch.full_like(e_t, float(self.ddim_sigmas[index]))
        sqrt_one_minus_at = torch.full_like(e_t, float(self.ddim_sqrt_one_minus_alphas[index]))
        pred_x0 = (x - sqrt_one_minus_at * e_t) / a_t.sqrt()
        if quantize_denoised:                     # ddim.py:260-261: pred_x0, _, *_ = self.model.first_stage_model.quantize(pred_x0)
            pred_x0 = self.model.quantize_first_stage(pred_x0)
        dir_xt = (1. - a_prev - sigma_t ** 2).sqrt() * e_t
        noise = sigma_t * noise * temperature
        if noise_dropout > 0.:
            noise = torch.nn.functional.dropout(noise, p=noise_dropout)
        x_prev = a_prev.sqrt() * pred_x0 + dir_xt + noise
        return x_prev, pred_x0

    # ---- image-to-image (ldm DDIMSampler.stochastic_encode / encode / decode; the reference's vendored ddim.py stops before them).
    # make_schedule(S) first, as in ldm.  "Level index i" is ddim_alphas[i]; DESIGN.md section 3 "Image-to-image" has the definitions.
    @staticmethod
    def img2img_steps(strength, total):
        """strength in (0, 1] -> the steps n of a `total`-step schedule an image-to-image call runs: min(total, max(1, int(strength *
        total))).  The start is noised to level index n - 1 and decode(t_start=n) begins there, so strength 1.0 runs the whole schedule."""
        strength = float(strength)
        if not 0. < strength <= 1.:
            raise ValueError(f"strength must lie in (0, 1], got {strength}")
        return min(int(total), max(1, int(strength * int(total))))

    def _level_index(self, what, name, v, lo):
        """An integer (or a tensor of equal integers, as ldm passes t) in [lo, total] / [lo, total - 1]."""
        if isinstance(v, torch.Tensor):
            flat = v.reshape(-1)
            if flat.numel() < 1 or not bool((flat == flat[0]).all()):
                raise ValueError(f"{what}: {name} must be one level for the whole batch")
            v = flat[0].item()
        total = self.ddim_timesteps.shape[0]
        hi = total if lo == 1 else total - 1
        if int(v) != v or not lo <= int(v) <= hi:
            raise ValueError(f"{what}: {name} must be an integer in [{lo}, {hi}] for this schedule of {total} timesteps, got {v}")
        return int(v)

    @staticmethod
    def _inpaint_mask(mask, shape):
        """A decode mask on the latent's device as the blend kernel reads it: fp32 [B, 1 | C, H, W] (a [1, ...] mask repeated over the batch)."""
        B, C, H, W = (int(v) for v in shape)
        m = torch.as_tensor(mask)
        if m.ndim != 4 or m.shape[0] not in (1, B) or m.shape[1] not in (1, C) or tuple(m.shape[2:]) != (H, W):
            raise ValueError(f"decode: mask must be [{B} | 1, 1 | {C}, {H}, {W}], got {tuple(m.shape)}")
        return m.float().expand(B, -1, -1, -1).contiguous()

    @torch.no_grad()
    def keep_known(self, x, x0, mask):
        """[native] x0 * mask + (1 - mask) * x on the blend kernel (sqrt_a = 1, sqrt_1ma = 0, no noise): what an inpainting call ends
        with, so that the known region of its result is x0 itself wherever the mask is 1."""
        x = x.to(self.model.device).float().contiguous()
        return self.model.ctx.op_masked_blend(x, x0.to(x.device).float().contiguous(), self._inpaint_mask(mask, x.shape).to(x.device), None,
                                              1.0, 0.0)

    def _level_scalars(self, a):
        """sqrt(a), sqrt(1 - a) in float64 from the fp32 alpha, as python floats (the native loops round them to fp32)."""
        a = float(a)
        return float(np.sqrt(a)), float(np.sqrt(1. - a))

    @torch.no_grad()
    def stochastic_encode(self, x0, t, use_original_steps=False, noise=None, noise_seed=None, noise_row0=0):
        """ldm stochastic_encode: sqrt(a_t[t]) x0 + sqrt(1 - a_t[t]) z for level index t.  noise_seed / noise_row0 [native]: z is the
        library's starting-latent normals of (seed, stream 0, step 0, noise_row0 + b), drawn in the kernel that applies them -- what a
        seeded sampling call starts from; no noise tensor exists.  Otherwise `noise`, or torch's generator as ldm does."""
        self._refuse_original_steps(use_original_steps)
        self._one_noise_source(noise_seed, noise, "noise")
        t = self._level_index("stochastic_encode", "t", t, 0)
        sa, s1m = self._level_scalars(self.ddim_alphas[t])
        if noise_seed is not None:
            return self.model.ctx.op_q_sample_seeded(x0.to(self.model.device).float().contiguous(), sa, s1m, noise_seed, row0=noise_row0)
        if noise is None:
            noise = torch.randn_like(x0)
        return np.float32(sa).item() * x0 + np.float32(s1m).item() * noise.to(x0.device)

    @torch.no_grad()
    def p_invert_ddim(self, x, c, t, index, unconditional_guidance_scale=1., unconditional_conditioning=None):
        """One inversion step of the per-step path: from level a_prev[index] up to a_t[index] with the model at `t` (encode passes the
        TARGET timestep ddim_timesteps[index]).  A guided step takes the model's apply_model_guided where it has one: the forward of the
        native loops (apply_model on the doubled batch runs other kernel configurations, and a step UP the schedule carries an eps
        difference on undamped where a sampling step contracts it), so the iterates of the per-step path are the native loop's.
        -> (x_next, pred_x0)."""
        if unconditional_guidance_scale > 1. and unconditional_conditioning is not None and hasattr(self.model, "apply_model_guided"):
            e_c, e_u = self.model.apply_model_guided(x, int(t.reshape(-1)[0]), c, unconditional_conditioning)
            e_t = e_u + unconditional_guidance_scale * (e_c - e_u)
        else:
            e_t = self._model_output(x, t, c, unconditional_conditioning if unconditional_guidance_scale > 1. else None,
                                     unconditional_guidance_scale)
        sa_c, s1m_c = self._level_scalars(self.ddim_alphas_prev[index])
        sa_n, s1m_n = self._level_scalars(self.ddim_alphas[index])
        full = lambda v: torch.full_like(e_t, float(np.float32(v)))
        pred_x0 = (x - full(s1m_c) * e_t) / full(sa_c)
        return full(sa_n) * pred_x0 + full(s1m_n) * e_t, pred_x0

    @_biased
    @torch.no_grad()
    def encode(self, x0, c, t_enc, use_original_steps=False, return_intermediates=None, unconditional_guidance_scale=1.,
               unconditional_conditioning=None, callback=None):
        """Deterministic DDIM inversion, t_enc steps up the schedule: step i moves the iterate from level a_prev[i] to a_t[i] with the
        UNet on the current iterate at the TARGET timestep ddim_timesteps[i] (ldm passes the loop index i as the timestep; DESIGN.md
        section 3 has the measurement behind the choice).  The result is at level index t_enc - 1: what decode(t_start=t_enc) expects.
        -> (x_next, out) as ldm: out['x_encoded'], out['intermediate_steps'], and with return_intermediates = k the iterates after the
        steps with i % max(t_enc // k, 1) == 0 or i == t_enc - 1 in out['intermediates'].  A callback (called with i) takes the
        per-step path; otherwise the loop runs in the library (rdm_ddim_encode)."""
        self._refuse_original_steps(use_original_steps)
        t_enc = self._level_index("encode", "t_enc", t_enc, 1)
        if unconditional_guidance_scale < 1.:
            raise ValueError("encode: unconditional_guidance_scale must be >= 1")
        c = self._unwrap(c, single="DDIM")
        uc = self._unwrap(unconditional_conditioning) if unconditional_guidance_scale > 1. else None
        if unconditional_guidance_scale > 1. and uc is None:
            raise ValueError("encode: unconditional_conditioning is required when unconditional_guidance_scale > 1")
        every = max(t_enc // int(return_intermediates), 1) if return_intermediates else None
        steps = [i for i in range(t_enc) if every is not None and (i % every == 0 or i == t_enc - 1)]
        print(f"Running DDIM inversion with {t_enc} timesteps")
        if callback is not None:
            x, inter = x0.to(self.model.device), []
            for i in range(t_enc):
                ts = torch.full((x.shape[0],), int(self.ddim_timesteps[i]), device=x.device, dtype=torch.long)
                x, _ = self.p_invert_ddim(x, c, ts, i, unconditional_guidance_scale, uc)
                if i in steps:
                    inter.append(x)
                callback(i)
        else:
            x, xi = self.model.ctx.ddim_encode(self.ddim_num_steps, t_enc, x0, c, uc, self.alphas_cumprod, scale=unconditional_guidance_scale,
                                               log_every_t=every or t_enc, want_intermediates=every is not None)
            inter = [] if xi is None else list(xi)
        out = {'x_encoded': x, 'intermediate_steps': steps}
        if return_intermediates:
            out['intermediates'] = inter
        return x.detach(), out

    @_biased
    @torch.no_grad()
    def decode(self, x_latent, cond, t_start, unconditional_guidance_scale=1., unconditional_conditioning=None, use_original_steps=False,
               callback=None, img_callback=None, eta=None, temperature=1., noise=None, noise_seed=None, noise_row0=0, log_every_t=100,
               return_intermediates=False, intermediates_to_cpu=False, mask=None, x0=None, q_noise=None):
        """ldm decode: x_latent is taken to be at level index t_start - 1 and the DDIM step runs at indices t_start - 1 ... 0 --
        t_start forwards; t_start = the schedule's length is ddim_sampling from x_T = x_latent.  [native] eta (default: make_schedule's),
        temperature, noise (a [t_start, B, C, H, W] stack), noise_seed / noise_row0 (step i of this call takes the library's (seed,
        stream 1, step i)), log_every_t and return_intermediates ((x_dec, intermediates) instead of x_dec) as in sample().  A callback
        takes the per-step path; otherwise the loop runs in the library (rdm_ddim_decode).
        mask / x0 / q_noise [native]: inpainting, as in sample() -- before every step the iterate becomes q_sample(x0, t) * mask +
        (1 - mask) * img (mask [B | 1, 1 | C, H, W] in [0, 1], 1 = keep the known latent x0); the loop is the library's rdm_ddim_inpaint.
        The known region's noise of step i is q_noise[i] (a [t_start, B, C, H, W] stack), with noise_seed the library's (seed, stream 0,
        step i + 1) drawn in the blend kernel, else torch's.  The result of the last step is not blended (DESIGN.md section 3
        "Inpainting")."""
        self._refuse_original_steps(use_original_steps)
        self._one_noise_source(noise_seed, noise)
        if mask is None and (x0 is not None or q_noise is not None):
            raise ValueError("decode: x0 / q_noise belong to an inpainting call: give a mask")
        if mask is not None:
            if x0 is None:
                raise ValueError("decode: a mask needs x0, the known latent")
            self._one_noise_source(noise_seed, q_noise, "q_noise stack")
        t_start = self._level_index("decode", "t_start", t_start, 1)
        if unconditional_guidance_scale < 1.:
            raise ValueError("decode: unconditional_guidance_scale must be >= 1")
        cond = self._unwrap(cond, single="DDIM")
        uc = self._unwrap(unconditional_conditioning) if unconditional_guidance_scale > 1. else None
        if unconditional_guidance_scale > 1. and uc is None:
            raise ValueError("decode: unconditional_conditioning is required when unconditional_guidance_scale > 1")
        if eta is None:
            eta = self.ddim_eta
        elif float(eta) != self.ddim_eta:
            self.make_schedule(self.ddim_num_steps, ddim_eta=eta, verbose=False)
        img = x_latent.to(self.model.device)
        print(f"Running DDIM Sampling with {t_start} timesteps")
        inpaint = {}
        if mask is not None:
            inpaint = dict(mask=self._inpaint_mask(mask, img.shape).to(img.device), x0=x0.to(img.device).float().contiguous(), q_noise=q_noise)
            if tuple(inpaint["x0"].shape) != tuple(img.shape):
                raise ValueError(f"decode: x0 must have the latent's shape {tuple(img.shape)}, got {tuple(x0.shape)}")
        if callback is not None or img_callback is not None:
            if mask is not None:
                inpaint["q_noise_seed"] = noise_seed
            z, inter = self._python_loop(cond, img, callback, img_callback, log_every_t, temperature, eta, unconditional_guidance_scale, uc,
                                         intermediates_to_cpu, noise=noise, noise_seed=noise_seed, noise_row0=noise_row0,
                                         ts_all=self.ddim_timesteps[:t_start], **inpaint)
            return (z, inter) if return_intermediates else z
        seeded = {} if noise_seed is None else dict(seed=noise_seed, row0=noise_row0)
        if eta != 0. and noise is None and noise_seed is None:
            noise = torch.randn((t_start,) + tuple(img.shape), device=img.device)
        if mask is not None:
            if q_noise is None and noise_seed is None:
                inpaint["q_noise"] = torch.randn((t_start,) + tuple(img.shape), device=img.device)
            z, xi, pi = self.model.ctx.ddim_inpaint(self.ddim_num_steps, t_start, img, inpaint["x0"], inpaint["mask"], cond, uc,
                                                    self.alphas_cumprod, eta=eta, scale=unconditional_guidance_scale, noise=noise,
                                                    q_noise=inpaint["q_noise"], log_every_t=log_every_t, temperature=temperature,
                                                    want_intermediates=return_intermediates, **seeded)
            return (z.detach(), self._intermediates(img, xi, pi, intermediates_to_cpu)) if return_intermediates else z.detach()
        z, xi, pi = self.model.ctx.ddim_decode(self.ddim_num_steps, t_start, img, cond, uc, self.alphas_cumprod, eta=eta,
                                               scale=unconditional_guidance_scale, noise=noise, log_every_t=log_every_t,
                                               temperature=temperature, want_intermediates=return_intermediates, **seeded)
        return (z.detach(), self._intermediates(img, xi, pi, intermediates_to_cpu)) if return_intermediates else z.detach()
