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
from .ddim import _SamplerBase


class UniPCSampler(_SamplerBase):
    def __init__(self, model, **kwargs):
        super().__init__(model, **kwargs)
        ac = model.alphas_cumprod.detach().float().cpu()
        assert ac.shape[0] == self.ddpm_num_timesteps, 'alphas have to be defined for each timestep'
        self.register_buffer('alphas_cumprod', ac)

    def make_nodes(self, S, skip_type="logSNR", timesteps=None):
        """[native] the node list: `timesteps` as given, or the library's grid of S steps (the grids of DPMSolverSampler)."""
        if timesteps is not None:
            return np.asarray(timesteps, dtype=np.int64).reshape(-1)
        return _lib.dpmpp_timesteps(S, self.alphas_cumprod, skip_type).astype(np.int64)

    @torch.no_grad()
    def sample(self, S, batch_size, shape, conditioning=None, callback=None, normals_sequence=None, img_callback=None,
               quantize_x0=False, eta=0., mask=None, x0=None, temperature=1., noise_dropout=0., score_corrector=None,
               corrector_kwargs=None, verbose=True, x_T=None, log_every_t=100, unconditional_guidance_scale=1.,
               unconditional_conditioning=None, order=2, variant="bh2", corrector=True, skip_type="logSNR", lower_order_final=True,
               timesteps=None, **kwargs):
        """`order` (1 | 2 | 3: the predictor's), `variant` ("bh1" | "bh2"), `corrector`, `skip_type` ("logSNR" | "time_uniform"),
        `lower_order_final` and `timesteps` (an explicit node list, strictly decreasing) are [native]."""
        if eta != 0:
            raise ValueError('eta must be 0 for UniPC (the solver is deterministic)')
        if mask is not None or x0 is not None:
            raise ValueError('UniPC has no inpainting form (the predictor-corrector keeps two iterates; mask / x0 are not supported): '
                             'use DDIMSampler, PLMSSampler or DPMSolverSampler for inpainting')
        if order not in (1, 2, 3):
            raise ValueError(f'UniPC order must be 1, 2 or 3, got {order!r}')
        if variant not in _lib.UNIPC_VARIANTS:
            raise ValueError(f'UniPC variant must be one of {sorted(_lib.UNIPC_VARIANTS)}, got {variant!r}')
        if unconditional_guidance_scale < 1.:
            raise ValueError('unconditional_guidance_scale must be >= 1')
        if conditioning is not None and not isinstance(conditioning, (dict, list)):
            if conditioning.shape[0] != batch_size:
                print(f"Warning: Got {conditioning.shape[0]} conditionings but batch-size is {batch_size}")
        cond = self._unwrap(conditioning, single="UniPC")
        uc = self._unwrap(unconditional_conditioning)
        nodes = self.make_nodes(S, skip_type, timesteps)
        n_steps = len(nodes) - 1
        device = self.model.device
        size = (batch_size,) + tuple(shape)
        img = torch.randn(size, device=device) if x_T is None else x_T.to(device)
        print(f"Running UniPC Sampling (order {order}, {variant}, corrector {'on' if corrector else 'off'}) with {n_steps} timesteps")
        guided = uc is not None and unconditional_guidance_scale != 1.
        scale = unconditional_guidance_scale if guided else 1.0
        solver = dict(order=order, variant=variant, corrector=bool(corrector), lower_order_final=bool(lower_order_final))
        if callback is not None or img_callback is not None or quantize_x0 or score_corrector is not None:
            return self._python_loop(nodes, cond, img, callback, img_callback, log_every_t, solver, quantize_x0, score_corrector,
                                     corrector_kwargs, scale, uc if guided else None)
        z, xi, pi = self.model.ctx.unipc_sample(nodes, img, cond, uc if guided else None, self.alphas_cumprod, scale=scale,
                                                log_every_t=log_every_t, want_intermediates=True, **solver)
        intermediates = {'x_inter': [img] + list(xi), 'pred_x0': [img] + list(pi)}
        return z.detach(), intermediates

    def _python_loop(self, nodes, cond, img, callback, img_callback, log_every_t, solver, quantize_denoised, score_corrector,
                     corrector_kwargs, scale, uc):
        """Per-step path of sample: native apply_model per forward, torch fp32 updates with the library's coefficients, in the
        kernel's association."""
        ac = self.alphas_cumprod.numpy()
        n_steps = len(nodes) - 1
        if n_steps < 1 or np.any(np.diff(nodes) >= 0) or nodes[0] >= ac.shape[0] or nodes[-1] < 0:
            raise ValueError(f"UniPC nodes must be strictly decreasing timesteps in [0, {ac.shape[0] - 1}], at least two")
        intermediates = {'x_inter': [img], 'pred_x0': [img]}
        b = img.shape[0]
        u, xc, hist = img, img, []                   # hist: m_{j-1}, m_{j-2}, m_{j-3}
        for j in range(n_steps):
            index = n_steps - 1 - j
            ts = torch.full((b,), int(nodes[j]), device=u.device, dtype=torch.long)
            if uc is None:
                e = self.model.apply_model(u, ts, cond)
            else:
                out = self.model.apply_model(torch.cat([u] * 2), torch.cat([ts] * 2), torch.cat([cond, uc]))
                e = out[b:] + scale * (out[:b] - out[b:])
            if score_corrector is not None:
                assert getattr(self.model, "parameterization", "eps") == "eps"
                e = score_corrector.modify_score(self.model, e, u, ts, cond, **(corrector_kwargs or {}))
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
            if callback: callback(j)
            if img_callback: img_callback(m, j)
            if self._logs(index, log_every_t, n_steps):
                intermediates['x_inter'].append(u)
                intermediates['pred_x0'].append(m)
        return u, intermediates
