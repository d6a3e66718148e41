"""SAMPLING ONLY — native counterpart of ldm's DPMSolverSampler (ldm/models/diffusion/dpm_solver/sampler.py; `--dpm_solver` in
ldm's txt2img script): DPM-Solver++(2M), the multistep data-prediction solver of Lu et al. 2022 ("DPM-Solver++: Fast Solver for
Guided Sampling of Diffusion Probabilistic Models"), here on INTEGER timesteps.

`sample` has ldm's signature and returns `(z, intermediates)` like PLMSSampler here.  The solver walks a strictly decreasing node list
nodes[0] > ... > nodes[n-1] of model timesteps with n - 1 UNet forwards (at nodes[0 .. n-2]) and ends at the noise level of
nodes[n-1].  With a = alphas_cumprod[t] in float64, alpha = sqrt(a), sigma = sqrt(1 - a), lambda = log(a / (1 - a)) / 2, step j from
s = nodes[j] to t = nodes[j+1] is

    m_j = (x - sigma_s eps) / alpha_s                 (eps guided: e_u + scale (e_c - e_u)),       h_j = lambda_t - lambda_s
    D   = (1 + 1/(2r)) m_j - (1/(2r)) m_{j-1},  r = h_{j-1} / h_j      when order == 2, j >= 1, not (lower_order_final and last step)
    D   = m_j                                                          otherwise
    x  <- (sigma_t / sigma_s) x - alpha_t expm1(-h_j) D

and order 1 is DDIM with eta = 0.  The node list comes from the library (rdm_dpmpp_timesteps): `skip_type="logSNR"` (uniform in
lambda from T - 1 to 0, rounded to timesteps; the grid this solver needs: on DDIM's grid it is barely better than DDIM) or
"time_uniform" (DDIM's S timesteps, then 0), or from `timesteps=`.  The logSNR grid may hold fewer than S steps when targets round to
the same timestep.  The loop runs inside librdm_hip (rdm_dpmpp_sample): K/V of the neighbours projected once per call, the
time-embedding table, the shared guidance prefix and the zero-context shortcut as in the DDIM loop, one fused update kernel per step.
Options that change the loop body per step (callbacks, mask / x0 inpainting, quantize_x0 through the native quantiser applied to m_j,
score_corrector) take the per-step path: native `apply_model`, torch fp32 update; it reads only `model.num_timesteps`,
`model.alphas_cumprod`, `model.device` and `model.apply_model` (and `model.q_sample` under a mask, when the model has one).  The solver
is deterministic: eta != 0 raises ValueError; `temperature` and `noise_dropout` have no effect.

DPMSolverSDESampler [native], at the end of the file, is the solver's stochastic form (SDE-DPM-Solver++(2M)) on the same surface.
"""
import math

import numpy as np
import torch

from ... import _lib
from .ddim import _SamplerBase
from .ddim import _biased


def dpmpp_coefficients(alphas_cumprod, s, t, h_prev=None):
    """Step s -> t in float64 from the fp32 alphas_cumprod: (alpha_s, sigma_s, c_x, c_0, c_1, h) with x_t = c_x x + c_0 m + c_1 m_prev.
    h_prev None: first-order step (c_1 = 0)."""
    a_s, a_t = float(alphas_cumprod[s]), float(alphas_cumprod[t])
    lam = lambda a: 0.5 * math.log(a / (1.0 - a))
    h = lam(a_t) - lam(a_s)
    g = -math.sqrt(a_t) * math.expm1(-h)
    c_x = math.sqrt(1.0 - a_t) / math.sqrt(1.0 - a_s)
    if h_prev is None:
        return math.sqrt(a_s), math.sqrt(1.0 - a_s), c_x, g, 0.0, h
    r = h_prev / h
    return math.sqrt(a_s), math.sqrt(1.0 - a_s), c_x, g * (1.0 + 1.0 / (2.0 * r)), -g / (2.0 * r), h


def dpmpp_sde_coefficients(alphas_cumprod, s, t, h_prev=None):
    """Step s -> t of SDE-DPM-Solver++ in float64 from the fp32 alphas_cumprod: (alpha_s, sigma_s, c_x, c_0, c_1, c_n, h) with
    x_t = c_x x + c_0 m + c_1 m_prev + c_n z (rdm_dpmpp_sde_sample's flattened form).  h_prev None: first-order step (c_1 = 0)."""
    a_s, a_t = float(alphas_cumprod[s]), float(alphas_cumprod[t])
    lam = lambda a: 0.5 * math.log(a / (1.0 - a))
    h = lam(a_t) - lam(a_s)
    q = -math.expm1(-2.0 * h)                   # 1 - exp(-2h)
    g = math.sqrt(a_t) * q
    c_x = math.sqrt(1.0 - a_t) / math.sqrt(1.0 - a_s) * math.exp(-h)
    c_n = math.sqrt(1.0 - a_t) * math.sqrt(q)
    if h_prev is None:
        return math.sqrt(a_s), math.sqrt(1.0 - a_s), c_x, g, 0.0, c_n, h
    r = h_prev / h
    return math.sqrt(a_s), math.sqrt(1.0 - a_s), c_x, g * (1.0 + 1.0 / (2.0 * r)), -g / (2.0 * r), c_n, h


class _NodeListSampler(_SamplerBase):
    """What DPMSolverSampler and UniPCSampler share: solvers over a strictly decreasing list of integer timesteps, one forward per step.
    A subclass gives NAME (as its messages spell it), its option checks, its native call and its per-step update."""
    NAME = None

    def __init__(self, model, **kwargs):
        super().__init__(model, **kwargs)
        ac = model.alphas_cumprod.detach().float().cpu()
        assert ac.shape[0] == self.ddpm_num_timesteps, 'alphas have to be defined for each timestep'
        self.register_buffer('alphas_cumprod', ac)

    def make_nodes(self, S, skip_type="logSNR", timesteps=None):
        """[native] the node list: `timesteps` as given, or the library's grid of S steps."""
        if timesteps is not None:
            return np.asarray(timesteps, dtype=np.int64).reshape(-1)
        return _lib.dpmpp_timesteps(S, self.alphas_cumprod, skip_type).astype(np.int64)

    def _prepare(self, S, batch_size, shape, conditioning, eta, x_T, scale, uc, skip_type, timesteps):
        """The preamble of `sample` -> the node list, the conditioning, the unconditional one (None unless guided), the guidance scale
        (1.0 unless guided), the start latent."""
        if eta != 0:
            raise ValueError(f'eta must be 0 for {self.NAME} (the solver is deterministic)')
        if scale < 1.:
            raise ValueError('unconditional_guidance_scale must be >= 1')
        self._warn_batch(conditioning, batch_size)
        cond = self._unwrap(conditioning, single=self.NAME)
        uc = self._unwrap(uc)
        nodes = self.make_nodes(S, skip_type, timesteps)
        device = self.model.device
        img = torch.randn((batch_size,) + tuple(shape), device=device) if x_T is None else x_T.to(device)
        guided = uc is not None and scale != 1.
        return nodes, cond, uc if guided else None, scale if guided else 1.0, img

    def _python_loop(self, nodes, cond, img, uc, scale, update, callback, img_callback, log_every_t, score_corrector, corrector_kwargs,
                     mask=None, x0=None, q_noise=None):
        """Per-step path of `sample`: native apply_model per forward, then update(j, x, eps) -> (the next UNet input, m_j): the
        solver's torch fp32 update with the library's coefficients."""
        n_steps = len(nodes) - 1
        T = self.alphas_cumprod.shape[0]
        if n_steps < 1 or np.any(np.diff(nodes) >= 0) or nodes[0] >= T or nodes[-1] < 0:
            raise ValueError(f"{self.NAME} nodes must be strictly decreasing timesteps in [0, {T - 1}], at least two")
        intermediates = {'x_inter': [img], 'pred_x0': [img]}
        for j in range(n_steps):
            ts = torch.full((img.shape[0],), int(nodes[j]), device=img.device, dtype=torch.long)
            if mask is not None:
                img = self._masked_blend(img, mask, x0, ts, None if q_noise is None else q_noise[j])
            img, m = update(j, img, self._model_output(img, ts, cond, uc, scale, score_corrector, corrector_kwargs))
            if callback: callback(j)
            if img_callback: img_callback(m, j)
            if self._logs(n_steps - 1 - j, log_every_t, n_steps):
                intermediates['x_inter'].append(img)
                intermediates['pred_x0'].append(m)
        return img, intermediates


class DPMSolverSampler(_NodeListSampler):
    NAME = "DPM-Solver++"

    @_biased
    @torch.no_grad()
    def sample(self, S, batch_size, shape, conditioning=None, callback=None, normals_sequence=None, img_callback=None,
               quantize_x0=False, eta=0., mask=None, x0=None, temperature=1., noise_dropout=0., score_corrector=None,
               corrector_kwargs=None, verbose=True, x_T=None, log_every_t=100, unconditional_guidance_scale=1.,
               unconditional_conditioning=None, order=2, skip_type="logSNR", lower_order_final=None, timesteps=None, noise_seed=None, noise_row0=0, **kwargs):
        """`noise_seed` / `noise_row0` [native]: without an x_T the starting latent is the library's own (DDIMSampler.sample); no per-step
        noise is drawn.  `order` (1 | 2), `skip_type` ("logSNR" | "time_uniform"), `lower_order_final` (None: on below 15 steps), `timesteps` (an
        explicit node list, strictly decreasing) and `q_noise` (explicit stack [steps, B, C, H, W] for q_sample of the masked region,
        per-step path) are [native]."""
        if order not in (1, 2):
            raise ValueError(f'DPM-Solver++ order must be 1 or 2, got {order!r}')
        x_T = self._seeded_start(x_T, (batch_size,) + tuple(shape), noise_seed, noise_row0)
        nodes, cond, uc, scale, img = self._prepare(S, batch_size, shape, conditioning, eta, x_T, unconditional_guidance_scale,
                                                    unconditional_conditioning, skip_type, timesteps)
        n_steps = len(nodes) - 1
        if lower_order_final is None:
            lower_order_final = n_steps < 15
        print(f"Running DPM-Solver++ Sampling (order {order}) with {n_steps} timesteps")
        if (callback is not None or img_callback is not None or quantize_x0 or mask is not None or x0 is not None or
                score_corrector is not None):
            return self._python_loop(nodes, cond, img, uc, scale, self._update(nodes, order, lower_order_final, quantize_x0), callback,
                                     img_callback, log_every_t, score_corrector, corrector_kwargs, mask, x0, kwargs.get("q_noise"))
        z, xi, pi = self.model.ctx.dpmpp_sample(nodes, img, cond, uc, self.alphas_cumprod, scale=scale, order=order,
                                                lower_order_final=lower_order_final, log_every_t=log_every_t, want_intermediates=True)
        return z.detach(), self._intermediates(img, xi, pi)

    def _update(self, nodes, order, lower_order_final, quantize_denoised):
        """The per-step path's update(j, x, eps) -> (x at node j + 1, m_j)."""
        ac = self.alphas_cumprod.numpy()
        f32 = lambda v: float(np.float32(v))
        m_prev, h_prev = None, None

        def update(j, x, e):
            nonlocal m_prev, h_prev
            second = order == 2 and j >= 1 and not (lower_order_final and j == len(nodes) - 2)
            alpha_s, sigma_s, c_x, c_0, c_1, h_prev = dpmpp_coefficients(ac, int(nodes[j]), int(nodes[j + 1]), h_prev if second else None)
            m = (x - f32(sigma_s) * e) / f32(alpha_s)
            if quantize_denoised:
                m = self.model.quantize_first_stage(m)
            x = f32(c_x) * x + f32(c_0) * m
            if second:
                x = x + f32(c_1) * m_prev
            m_prev = m
            return x, m
        return update


class DPMSolverSDESampler(_NodeListSampler):
    """[native] SDE-DPM-Solver++(2M): the `sde-dpmsolver++` multistep update of Lu et al.'s reference implementation -- a stochastic sampler
    at DPM-Solver++'s step counts, on the same node lists, order rule and options as DPMSolverSampler.  Step j from s to t adds fresh noise:

        g  = alpha_t (1 - exp(-2 h_j))
        x <- (sigma_t / sigma_s) exp(-h_j) x + g m_j  [+ (g / (2r)) (m_j - m_{j-1}) on a second-order step]  + sigma_t sqrt(1 - exp(-2 h_j)) z_j

    so the sample forgets its start, which the ODE solvers cannot.  The noise is not scaled by an eta: eta != 0 raises.  z_j comes from
    `noise=` (a [steps, B, C, H, W] stack), from the library's counter-based generator under `noise_seed` / `noise_row0` (stream 1, step j,
    rows noise_row0 .. -- generated in the step kernel, no stack exists, and a row's sample does not depend on how a batch is sharded; the
    starting latent, when no x_T is given, is the library's too), or else from torch's generator the way DDIMSampler draws its stack for
    eta > 0.  The loop runs inside librdm_hip (rdm_dpmpp_sde_sample); the per-step options of
    DPMSolverSampler take the per-step path here too."""
    NAME = "SDE-DPM-Solver++"

    @_biased
    @torch.no_grad()
    def sample(self, S, batch_size, shape, conditioning=None, callback=None, normals_sequence=None, img_callback=None,
               quantize_x0=False, eta=0., mask=None, x0=None, temperature=1., noise_dropout=0., score_corrector=None,
               corrector_kwargs=None, verbose=True, x_T=None, log_every_t=100, unconditional_guidance_scale=1.,
               unconditional_conditioning=None, order=2, skip_type="logSNR", lower_order_final=None, timesteps=None, noise_seed=None, noise_row0=0,
               noise=None, **kwargs):
        """As DPMSolverSampler.sample, plus `noise` [native]: the explicit stack [steps, B, C, H, W] of the steps' z_j (consumed in loop
        order).  `noise_seed` / `noise_row0` select the library's generator for the starting latent (when no x_T is given) AND for z_j;
        a stack and a seed together raise."""
        if eta != 0:
            raise ValueError(f"eta must be 0 for {self.NAME}: this solver's noise is not scaled by eta (it is the SDE's own)")
        if order not in (1, 2):
            raise ValueError(f'{self.NAME} order must be 1 or 2, got {order!r}')
        self._one_noise_source(noise_seed, noise)
        x_T = self._seeded_start(x_T, (batch_size,) + tuple(shape), noise_seed, noise_row0)
        nodes, cond, uc, scale, img = self._prepare(S, batch_size, shape, conditioning, 0., x_T, unconditional_guidance_scale,
                                                    unconditional_conditioning, skip_type, timesteps)
        n_steps = len(nodes) - 1
        if lower_order_final is None:
            lower_order_final = n_steps < 15
        if noise is not None and tuple(noise.shape) != (n_steps,) + tuple(img.shape):
            raise ValueError(f"{self.NAME} noise stack must be {(n_steps,) + tuple(img.shape)} (one z per step), got {tuple(noise.shape)}")
        if noise is None and noise_seed is None:
            noise = torch.randn((n_steps,) + tuple(img.shape), device=img.device)
        print(f"Running SDE-DPM-Solver++ Sampling (order {order}) with {n_steps} timesteps")
        if (callback is not None or img_callback is not None or quantize_x0 or mask is not None or x0 is not None or
                score_corrector is not None):
            draw = ((lambda j: noise[j].to(img.device)) if noise is not None else
                    (lambda j: self._device_randn(img.shape, noise_seed, noise_row0, step=j, stream=1)))
            return self._python_loop(nodes, cond, img, uc, scale, self._update(nodes, order, lower_order_final, quantize_x0, draw), callback,
                                     img_callback, log_every_t, score_corrector, corrector_kwargs, mask, x0, kwargs.get("q_noise"))
        seeded = {} if noise_seed is None else dict(seed=noise_seed, row0=noise_row0)
        z, xi, pi = self.model.ctx.dpmpp_sde_sample(nodes, img, cond, uc, self.alphas_cumprod, scale=scale, order=order,
                                                    lower_order_final=lower_order_final, noise=noise, log_every_t=log_every_t,
                                                    want_intermediates=True, **seeded)
        return z.detach(), self._intermediates(img, xi, pi)

    def _update(self, nodes, order, lower_order_final, quantize_denoised, draw):
        """The per-step path's update(j, x, eps) -> (x at node j + 1, m_j); draw(j) -> z_j."""
        ac = self.alphas_cumprod.numpy()
        f32 = lambda v: float(np.float32(v))
        m_prev, h_prev = None, None

        def update(j, x, e):
            nonlocal m_prev, h_prev
            second = order == 2 and j >= 1 and not (lower_order_final and j == len(nodes) - 2)
            alpha_s, sigma_s, c_x, c_0, c_1, c_n, h_prev = dpmpp_sde_coefficients(ac, int(nodes[j]), int(nodes[j + 1]), h_prev if second else None)
            m = (x - f32(sigma_s) * e) / f32(alpha_s)
            if quantize_denoised:
                m = self.model.quantize_first_stage(m)
            x = f32(c_x) * x + f32(c_0) * m
            if second:
                x = x + f32(c_1) * m_prev
            x = x + f32(c_n) * draw(j)
            m_prev = m
            return x, m
        return update
