"""SAMPLING ONLY — UniPC (Zhao et al. 2023, "UniPC: A Unified Predictor-Corrector Framework for Fast Sampling of Diffusion Models"):
the multistep data-prediction solver of DPMSolverSampler plus a corrector that reuses the forward the next step needs anyway, here on
INTEGER timesteps.  [native]: written from the paper's algorithm; ldm-style `uni_pc.py` has this `sample` surface.

`sample` has DPMSolverSampler's signature and returns `(z, intermediates)`.  The solver walks a strictly decreasing node list
nodes[0] > ... > nodes[n] of model timesteps with n UNet forwards (at nodes[0 .. n-1]) and ends at the noise level of nodes[n].
u_j is the UNet input at node j (u_0 = x_0 = x_T), m_j = (u_j - sigma_j eps_j) / alpha_j with the guided eps.  Step s (ending at node s)
has order p = min(order, s), with lower_order_final also at most n + 1 - s:

    h = lambda_s - lambda_{s-1},  hh = -h,  phi_1 = expm1(hh),  B = hh ("bh1") | expm1(hh) ("bh2")
    r_i = (lambda_{s-1-i} - lambda_{s-1}) / h (i < p),  r_p = 1,   D_i = (m_{s-1-i} - m_{s-1}) / r_i
    base = (sigma_s / sigma_{s-1}) x_{s-1} - alpha_s phi_1 m_{s-1}
    u_s = base - alpha_s B sum_{i<p} rho^p_i D_i                                       (predicted: the next UNet input)
    x_s = base - alpha_s B (sum_{i<p} rho^c_i D_i + rho^c_p (m_s - m_{s-1}))            (corrected, m_s from the forward at u_s)

with the weights rho of include/rdm_hip.h (rdm_unipc_sample).  m_s comes from the PREDICTED u_s, so the corrector costs no forward:
order 2 with the corrector is third order at DPM-Solver++(2M)'s price.  With `corrector=False`, order 2 / "bh2" IS DPM-Solver++(2M) and
order 1 is DDIM with eta = 0.  The last node is not corrected (no forward there): z = u_n.

The loop runs inside librdm_hip (rdm_unipc_sample): K/V of the neighbours projected once per call, the time-embedding table, the shared
guidance prefix and the zero-context shortcut as in the DDIM loop, one fused predict-and-correct kernel per step; the scalars come from
rdm_unipc_coefficients in float64.  Options that change the loop body per step (callbacks, quantize_x0 through the native quantiser
applied to m_j, score_corrector) take the per-step path: native `apply_model`, torch fp32 update with the same coefficients; it reads
only `model.num_timesteps`, `model.alphas_cumprod`, `model.device` and `model.apply_model`.  The solver is deterministic: eta != 0
raises ValueError; `temperature` and `noise_dropout` have no effect.  There is no inpainting form (mask / x0 raise ValueError): the
corrector would mix a blended UNet input with an unblended kept iterate.
"""
import numpy as np
import torch

from ... import _lib
from .ddim import _biased
from .dpm_solver import _NodeListSampler


class UniPCSampler(_NodeListSampler):
    NAME = "UniPC"

    @_biased
    @torch.no_grad()
    def sample(self, S, batch_size, shape, conditioning=None, callback=None, normals_sequence=None, img_callback=None,
               quantize_x0=False, eta=0., mask=None, x0=None, temperature=1., noise_dropout=0., score_corrector=None,
               corrector_kwargs=None, verbose=True, x_T=None, log_every_t=100, unconditional_guidance_scale=1.,
               unconditional_conditioning=None, order=2, variant="bh2", corrector=True, skip_type="logSNR", lower_order_final=True,
               timesteps=None, noise_seed=None, noise_row0=0, **kwargs):
        """`noise_seed` / `noise_row0` [native]: without an x_T the starting latent is the library's own (DDIMSampler.sample); no per-step
        noise is drawn.  `order` (1 | 2 | 3: the predictor's), `variant` ("bh1" | "bh2"), `corrector`, `skip_type` ("logSNR" | "time_uniform"),
        `lower_order_final` and `timesteps` (an explicit node list, strictly decreasing) are [native]."""
        if mask is not None or x0 is not None:
            raise ValueError('UniPC has no inpainting form (the predictor-corrector keeps two iterates; mask / x0 are not supported): '
                             'use DDIMSampler, PLMSSampler or DPMSolverSampler for inpainting')
        if order not in (1, 2, 3):
            raise ValueError(f'UniPC order must be 1, 2 or 3, got {order!r}')
        if variant not in _lib.UNIPC_VARIANTS:
            raise ValueError(f'UniPC variant must be one of {sorted(_lib.UNIPC_VARIANTS)}, got {variant!r}')
        x_T = self._seeded_start(x_T, (batch_size,) + tuple(shape), noise_seed, noise_row0)
        nodes, cond, uc, scale, img = self._prepare(S, batch_size, shape, conditioning, eta, x_T, unconditional_guidance_scale,
                                                    unconditional_conditioning, skip_type, timesteps)
        print(f"Running UniPC Sampling (order {order}, {variant}, corrector {'on' if corrector else 'off'}) with {len(nodes) - 1} timesteps")
        solver = dict(order=order, variant=variant, corrector=bool(corrector), lower_order_final=bool(lower_order_final))
        if callback is not None or img_callback is not None or quantize_x0 or score_corrector is not None:
            return self._python_loop(nodes, cond, img, uc, scale, self._update(nodes, solver, quantize_x0), callback, img_callback,
                                     log_every_t, score_corrector, corrector_kwargs)
        z, xi, pi = self.model.ctx.unipc_sample(nodes, img, cond, uc, self.alphas_cumprod, scale=scale, log_every_t=log_every_t,
                                                want_intermediates=True, **solver)
        return z.detach(), self._intermediates(img, xi, pi)

    def _update(self, nodes, solver, quantize_denoised):
        """The per-step path's update(j, u_j, eps) -> (u_{j+1}, m_j), in the kernel's association."""
        ac = self.alphas_cumprod.numpy()
        xc, hist = None, []                          # the kept (corrected) iterate; m_{j-1}, m_{j-2}, m_{j-3}

        def update(j, u, e):
            nonlocal xc, hist
            co = _lib.unipc_coefficients(nodes, ac, j, **solver)
            alpha, sigma, a_x, a_t, a_1, a_2, a_3, b_x, b_0, b_1, b_2 = (float(np.float32(v)) for v in co[:11])
            order_c, order_p = int(co[11]), int(co[12])
            m = (u - sigma * e) / alpha
            if quantize_denoised:
                m = self.model.quantize_first_stage(m)
            if order_c >= 1:
                xc = a_x * xc + a_t * m
                for a_i, h in zip((a_1, a_2, a_3)[:order_c], hist):
                    xc = xc + a_i * h
            else:
                xc = u
            u = b_x * xc + b_0 * m
            for b_i, h in zip((b_1, b_2)[:order_p - 1], hist):
                u = u + b_i * h
            hist = [m] + hist[:2]
            return u, m
        return update
