"""SAMPLING ONLY — native counterpart of ldm's PLMSSampler (ldm/models/diffusion/plms.py, pseudo linear multistep; `--plms` in
ldm's txt2img script).

Same constructor, `make_schedule`, `sample`, `plms_sampling`, `p_sample_plms` signatures and return values.  The schedule is
DDIM's with eta = 0 (make_schedule raises ValueError for any other eta); the first step is a pseudo improved Euler step (two UNet
forwards), later steps combine the guided eps with up to three earlier ones, so S' timesteps cost S' + 1 forwards.  The loop runs
inside librdm_hip (rdm_plms_sample): K/V of the neighbours projected once per call, the time-embedding table, the shared guidance
prefix and the zero-context shortcut as in the DDIM loop.  Options that change the loop body per step (callbacks, mask / x0
inpainting, quantize_x0 through the native quantiser, score_corrector, a timestep subset) take the per-step path: native
`apply_model`, torch fp32 update; it reads only `model.num_timesteps`, `model.alphas_cumprod`, `model.device` and
`model.apply_model` (and `model.q_sample` under a mask, when the model has one).  sigma_t is 0, so `temperature` and `noise_dropout` have no effect (as in ldm).  ddim_use_original_steps raises
NotImplementedError, for the reason given in ddim.py.
"""
import numpy as np
import torch

from .ddim import _SamplerBase
from .ddim import _biased


class PLMSSampler(_SamplerBase):
    def make_schedule(self, ddim_num_steps, ddim_discretize="uniform", ddim_eta=0., verbose=True):
        if ddim_eta != 0:
            raise ValueError('ddim_eta must be 0 for PLMS')
        self.ddim_num_steps = ddim_num_steps            # [native] the S the library rebuilds this schedule from
        super().make_schedule(ddim_num_steps, ddim_discretize, ddim_eta, verbose)

    @_biased
    @torch.no_grad()
    def sample(self, S, batch_size, shape, conditioning=None, callback=None, normals_sequence=None, img_callback=None,
               quantize_x0=False, eta=0., mask=None, x0=None, temperature=1., noise_dropout=0., score_corrector=None,
               corrector_kwargs=None, verbose=True, x_T=None, log_every_t=100, unconditional_guidance_scale=1.,
               unconditional_conditioning=None, noise_seed=None, noise_row0=0, **kwargs):
        """`noise_seed` / `noise_row0` [native]: without an x_T the starting latent is the library's own (DDIMSampler.sample); PLMS draws
        no per-step noise."""
        self._warn_batch(conditioning, batch_size)
        self.make_schedule(ddim_num_steps=S, ddim_eta=eta, verbose=verbose)
        size = (batch_size,) + tuple(shape)
        x_T = self._seeded_start(x_T, size, noise_seed, noise_row0)
        return self.plms_sampling(conditioning, size, callback=callback, img_callback=img_callback,
                                  quantize_denoised=quantize_x0, mask=mask, x0=x0, ddim_use_original_steps=False,
                                  noise_dropout=noise_dropout, temperature=temperature, score_corrector=score_corrector,
                                  corrector_kwargs=corrector_kwargs, x_T=x_T, log_every_t=log_every_t,
                                  unconditional_guidance_scale=unconditional_guidance_scale,
                                  unconditional_conditioning=unconditional_conditioning, q_noise=kwargs.get("q_noise"))

    @torch.no_grad()
    def plms_sampling(self, cond, shape, x_T=None, ddim_use_original_steps=False, callback=None, timesteps=None,
                      quantize_denoised=False, mask=None, x0=None, img_callback=None, log_every_t=100, temperature=1.,
                      noise_dropout=0., score_corrector=None, corrector_kwargs=None, unconditional_guidance_scale=1.,
                      unconditional_conditioning=None, q_noise=None):
        """`q_noise` [native]: optional explicit stack [steps, B, C, H, W] for q_sample of the masked region (per-step path)."""
        self._refuse_original_steps(ddim_use_original_steps)
        cond = self._unwrap(cond, single="PLMS")
        unconditional_conditioning = self._unwrap(unconditional_conditioning)
        device = self.model.device
        img = torch.randn(shape, device=device) if x_T is None else x_T.to(device)
        per_step = (callback is not None or img_callback is not None or quantize_denoised or mask is not None or x0 is not None or
                    score_corrector is not None or timesteps is not None)
        if per_step:
            return self._python_loop(cond, img, callback, img_callback, log_every_t, timesteps, quantize_denoised, mask, x0,
                                     score_corrector, corrector_kwargs, unconditional_guidance_scale, unconditional_conditioning,
                                     q_noise)
        print(f"Running PLMS Sampling with {self.ddim_timesteps.shape[0]} timesteps")
        guided = unconditional_conditioning is not None and unconditional_guidance_scale != 1.
        z, xi, pi = self.model.ctx.plms_sample(self.ddim_num_steps, img, cond,
                                               unconditional_conditioning if guided else None, self.alphas_cumprod,
                                               scale=unconditional_guidance_scale if guided else 1.0, log_every_t=log_every_t,
                                               want_intermediates=True)
        return z.detach(), self._intermediates(img, xi, pi)

    def _python_loop(self, cond, img, callback, img_callback, log_every_t, timesteps, quantize_denoised, mask, x0, score_corrector,
                     corrector_kwargs, scale, uc, q_noise):
        """Per-step path of plms_sampling: native apply_model per forward, torch fp32 update."""
        timesteps = self._timestep_subset(timesteps)
        intermediates = {'x_inter': [img], 'pred_x0': [img]}
        time_range = np.flip(timesteps)
        total_steps = timesteps.shape[0]
        print(f"Running PLMS Sampling with {total_steps} timesteps")
        b = img.shape[0]
        old_eps = []
        for i, step in enumerate(time_range):
            index = total_steps - i - 1
            ts = torch.full((b,), int(step), device=img.device, dtype=torch.long)
            ts_next = torch.full((b,), int(time_range[min(i + 1, len(time_range) - 1)]), device=img.device, dtype=torch.long)
            if mask is not None:
                img = self._masked_blend(img, mask, x0, ts, None if q_noise is None else q_noise[i])
            img, pred_x0, e_t = self.p_sample_plms(img, cond, ts, index=index, quantize_denoised=quantize_denoised,
                                                   score_corrector=score_corrector, corrector_kwargs=corrector_kwargs,
                                                   unconditional_guidance_scale=scale, unconditional_conditioning=uc,
                                                   old_eps=old_eps, t_next=ts_next)
            old_eps.append(e_t)
            if len(old_eps) >= 4:
                old_eps.pop(0)
            if callback: callback(i)
            if img_callback: img_callback(pred_x0, i)
            if self._logs(index, log_every_t, total_steps):
                intermediates['x_inter'].append(img)
                intermediates['pred_x0'].append(pred_x0)
        return img, intermediates

    @torch.no_grad()
    def p_sample_plms(self, x, c, t, index, repeat_noise=False, use_original_steps=False, quantize_denoised=False,
                      temperature=1., noise_dropout=0., score_corrector=None, corrector_kwargs=None,
                      unconditional_guidance_scale=1., unconditional_conditioning=None, old_eps=None, t_next=None):
        if use_original_steps:
            raise NotImplementedError("use_original_steps: dead in the reference (ddim.py:249)")
        b = x.shape[0]

        def get_model_output(x, t):
            return self._model_output(x, t, c, unconditional_conditioning, unconditional_guidance_scale, score_corrector, corrector_kwargs,
                                      uncond_first=True)

        def get_x_prev_and_pred_x0(e_t, index):
            # sigma_t = 0 (eta = 0): dir_xt = (1 - a_prev - sigma_t**2).sqrt() * e_t and a zero noise term, as in ldm
            a_t = torch.full((b, 1, 1, 1), float(self.ddim_alphas[index]), device=x.device)
            a_prev = torch.full((b, 1, 1, 1), float(self.ddim_alphas_prev[index]), device=x.device)
            sqrt_one_minus_at = torch.full((b, 1, 1, 1), float(self.ddim_sqrt_one_minus_alphas[index]), device=x.device)
            pred_x0 = (x - sqrt_one_minus_at * e_t) / a_t.sqrt()
            if quantize_denoised:
                pred_x0 = self.model.quantize_first_stage(pred_x0)
            dir_xt = (1. - a_prev).sqrt() * e_t
            x_prev = a_prev.sqrt() * pred_x0 + dir_xt
            return x_prev, pred_x0

        e_t = get_model_output(x, t)
        if len(old_eps) == 0:
            # first step: pseudo improved Euler, a second forward at t_next
            x_prev, pred_x0 = get_x_prev_and_pred_x0(e_t, index)
            e_t_next = get_model_output(x_prev, t_next)
            e_t_prime = (e_t + e_t_next) / 2
        elif len(old_eps) == 1:
            # linear multistep (Adams-Bashforth coefficients) of order 2, 3, 4
            e_t_prime = (3 * e_t - old_eps[-1]) / 2
        elif len(old_eps) == 2:
            e_t_prime = (23 * e_t - 16 * old_eps[-1] + 5 * old_eps[-2]) / 12
        else:
            e_t_prime = (55 * e_t - 59 * old_eps[-1] + 37 * old_eps[-2] - 9 * old_eps[-3]) / 24
        x_prev, pred_x0 = get_x_prev_and_pred_x0(e_t_prime, index)
        return x_prev, pred_x0, e_t
