"""Self-contained schedulers with the interface ``LattePipeline`` uses (``set_timesteps``, ``timesteps``,
``init_noise_sigma``, ``scale_model_input``, ``step(...)[0]``, ``order``).

``sample/sample_t2x.py:43-114`` builds the scheduler from diffusers (``DDIMScheduler.from_pretrained(..., beta_start,
beta_end, beta_schedule, variance_type, clip_sample=False)``); diffusers is not available offline, so any object with this
interface can be passed to the pipeline and THIS class exists for self-contained runs and tests.  It restates the published
DDIM update (Song et al. 2020, eq. 12) with diffusers' "leading" timestep spacing; it is memory-derived and NOT pinned
against diffusers.  Host-side fp64 tables, a handful of elementwise torch ops per step on the latents: plumbing, not the
hot path (the denoiser call is).

The other four classes -- ``EulerDiscreteScheduler``, ``EulerAncestralDiscreteScheduler``, ``HeunDiscreteScheduler`` and
``DPMSolverMultistepScheduler`` (the ``sample_method`` names of ``sample_t2x.py:51-100`` that have a linear update) -- restate the
published updates (Karras et al. 2022, algorithms 1-2; Lu et al. 2022, DPM-Solver++ 2M) the same way: memory-derived, NOT pinned
against diffusers.  Each one also describes its chain as a table, ``engine_plan()``: one row of ``PLAN_COLS`` doubles per denoiser
evaluation (include/latte_amd.h: latte_t2v_guided_linear_loop), which is what lets ``LattePipeline`` run the whole guided chain
inside the engine.  ``DDIMInverseScheduler`` walks the DDIM chain the other way (``LattePipeline.invert``) as the same kind of table.
``timestep_spacing`` is "leading" (the DDIM stand-in's) or "trailing"; "linspace" is refused: it gives fractional
timesteps and interpolated sigmas, and the engine's timestep input is int64 (``LatteT2V.forward`` truncates).

Notation: abar_i = alphas_cumprod at the i-th timestep of the set, abar = 1 after the last one.  The k-diffusion family (Euler,
Euler-ancestral, Heun) carries x~ = x / sqrt(abar) with sigma_i = sqrt((1 - abar_i) / abar_i): ``init_noise_sigma`` =
sqrt(sigma_0^2 + 1), model input x~ / sqrt(sigma_i^2 + 1).  DPM-Solver++ carries x itself.
"""
import numpy as np
import torch


class DDIMScheduler:
    order = 1
    init_noise_sigma = 1.0

    def __init__(self, num_train_timesteps=1000, beta_start=0.0001, beta_end=0.02, beta_schedule="linear", clip_sample=False,
                 set_alpha_to_one=True, steps_offset=0, **unused):
        if beta_schedule == "linear":
            betas = np.linspace(beta_start, beta_end, num_train_timesteps, dtype=np.float64)
        elif beta_schedule == "scaled_linear":
            betas = np.linspace(beta_start ** 0.5, beta_end ** 0.5, num_train_timesteps, dtype=np.float64) ** 2
        else:
            raise ValueError(f"unsupported beta_schedule {beta_schedule!r}")
        self.alphas_cumprod = np.cumprod(1.0 - betas)
        self.final_alpha_cumprod = 1.0 if set_alpha_to_one else float(self.alphas_cumprod[0])
        self.num_train_timesteps, self.clip_sample, self.steps_offset = num_train_timesteps, clip_sample, steps_offset
        self.num_inference_steps = None
        self.timesteps = torch.arange(num_train_timesteps - 1, -1, -1)

    def set_timesteps(self, num_inference_steps, device=None):
        step_ratio = self.num_train_timesteps // num_inference_steps                       # "leading" spacing
        ts = (np.arange(0, num_inference_steps) * step_ratio).round()[::-1].copy().astype(np.int64) + self.steps_offset
        self.num_inference_steps = num_inference_steps
        self.timesteps = torch.from_numpy(ts).to(device)

    def scale_model_input(self, sample, timestep=None):
        return sample

    def step(self, model_output, timestep, sample, eta=0.0, generator=None, return_dict=True):
        t = int(timestep)
        prev_t = t - self.num_train_timesteps // self.num_inference_steps
        a_t = float(self.alphas_cumprod[t])
        a_prev = float(self.alphas_cumprod[prev_t]) if prev_t >= 0 else self.final_alpha_cumprod
        x0 = (sample - (1.0 - a_t) ** 0.5 * model_output) / a_t ** 0.5
        if self.clip_sample:
            x0 = x0.clamp(-1.0, 1.0)
        sigma = eta * ((1.0 - a_prev) / (1.0 - a_t)) ** 0.5 * (1.0 - a_t / a_prev) ** 0.5
        eps = (sample - a_t ** 0.5 * x0) / (1.0 - a_t) ** 0.5 if self.clip_sample else model_output
        prev = a_prev ** 0.5 * x0 + (1.0 - a_prev - sigma ** 2) ** 0.5 * eps
        if eta > 0:
            noise = torch.randn(model_output.shape, generator=generator, device=model_output.device, dtype=model_output.dtype)
            prev = prev + sigma * noise
        return (prev,) if not return_dict else type("DDIMSchedulerOutput", (), {"prev_sample": prev, "pred_original_sample": x0})()


PLAN_COLS = 12
# columns of an engine_plan() row (include/latte_amd.h: LATTE_T2V_PLAN_COLS)
P_T, P_IN, P_MX, P_MEPS, P_CX, P_C0, P_C1, P_C2, P_C3, P_CN, P_PUSH, P_RSV = range(PLAN_COLS)


def draw_noise(shape, generator, device, dtype):
    """The one ``torch.randn`` call of a stochastic step: on the generator's device (a CPU generator serves a GPU chain, as in
    ``LattePipeline.prepare_latents``), then moved.  The pipeline's fused branch draws through this too, so both consume one stream."""
    gdev = generator.device if generator is not None else device
    return torch.randn(tuple(shape), generator=generator, device=gdev, dtype=dtype).to(device)


class _LinearScheduler:
    """Shared part of the four samplers: beta tables, timestep spacing, the step index, and the two views of one chain --
    ``step`` (diffusers interface, Python-float coefficients times the tensors) and ``engine_plan`` (the same coefficients as a
    table).  Subclasses fill ``self._rows`` ([n_evals, PLAN_COLS] float64) and ``self._eval_timesteps`` in ``_build``."""
    order = 1

    def __init__(self, num_train_timesteps=1000, beta_start=0.0001, beta_end=0.02, beta_schedule="linear",
                 timestep_spacing="leading", steps_offset=0, **unused):
        if beta_schedule == "linear":
            betas = np.linspace(beta_start, beta_end, num_train_timesteps, dtype=np.float64)
        elif beta_schedule == "scaled_linear":
            betas = np.linspace(beta_start ** 0.5, beta_end ** 0.5, num_train_timesteps, dtype=np.float64) ** 2
        else:
            raise ValueError(f"unsupported beta_schedule {beta_schedule!r}")
        if timestep_spacing == "linspace":
            raise ValueError("timestep_spacing='linspace' gives fractional timesteps and interpolated sigmas; the engine's timestep "
                             "input is int64 (LatteT2V.forward truncates), so only 'leading' and 'trailing' are offered")
        if timestep_spacing not in ("leading", "trailing"):
            raise ValueError(f"unsupported timestep_spacing {timestep_spacing!r}")
        self.alphas_cumprod = np.cumprod(1.0 - betas)
        self.num_train_timesteps, self.timestep_spacing, self.steps_offset = num_train_timesteps, timestep_spacing, steps_offset
        self.num_inference_steps = None
        # no chain until set_timesteps (as the DDIM stand-in): every trained timestep, and sigma of the noisiest one for init_noise_sigma
        self.timesteps = torch.arange(num_train_timesteps - 1, -1, -1)
        self._sigmas = np.array([((1.0 - self.alphas_cumprod[-1]) / self.alphas_cumprod[-1]) ** 0.5, 0.0])
        self._rows, self._step_index = None, 0

    # ------------------------------------------------------------------ tables
    def _spaced(self, n):
        T = self.num_train_timesteps
        if n < 1 or n > T:
            raise ValueError(f"num_inference_steps must be in [1, {T}]")
        if self.timestep_spacing == "leading":
            ts = (np.arange(0, n) * (T // n)).round()[::-1].copy().astype(np.int64) + self.steps_offset
        else:
            ts = np.round(np.arange(T, 0, -T / n)).astype(np.int64) - 1
        if ts.min() < 0 or ts.max() >= T:
            raise ValueError("timesteps leave the trained range (steps_offset too large)")
        return ts

    def _own_timesteps(self, timesteps, alphas_cumprod_at):
        """The checked (timesteps, abar at them) of ``set_timesteps(timesteps=..., alphas_cumprod_at=...)``."""
        if timesteps is None or alphas_cumprod_at is None:
            raise ValueError("timesteps= and alphas_cumprod_at= go together")
        ts = np.asarray(timesteps)
        ab = np.asarray(alphas_cumprod_at, dtype=np.float64)
        if ts.ndim != 1 or ts.size < 1 or not np.all(ts == np.floor(ts)) or ts.min() < 0:
            raise ValueError("timesteps must be a non-empty list of non-negative integers")
        ts = ts.astype(np.int64)
        if ab.shape != ts.shape:
            raise ValueError(f"alphas_cumprod_at has {ab.size} entries for {ts.size} timesteps")
        if np.any(np.diff(ts) >= 0):
            raise ValueError("timesteps must be distinct and descending")
        if not np.all(np.isfinite(ab)) or np.any(ab <= 0.0) or np.any(ab > 1.0):
            raise ValueError("alphas_cumprod_at must lie in (0, 1]")
        return ts, ab

    def set_timesteps(self, num_inference_steps=None, device=None, *, timesteps=None, alphas_cumprod_at=None):
        """``set_timesteps(n)``: n timesteps of the trained range by ``timestep_spacing``.  ``set_timesteps(timesteps=ts,
        alphas_cumprod_at=ab)``: the chain on a caller's own timesteps -- descending distinct integers with abar AT them (a respaced
        diffusion's ``timestep_map`` and ``alphas_cumprod``; the gaps need not be uniform, the scheduler's own beta table is not consulted);
        it ends at abar = 1 behind the last one all the same."""
        if timesteps is not None or alphas_cumprod_at is not None:
            ts, abar = self._own_timesteps(timesteps, alphas_cumprod_at)
            if num_inference_steps is not None and num_inference_steps != len(ts):
                raise ValueError(f"num_inference_steps = {num_inference_steps} for {len(ts)} timesteps")
            num_inference_steps = len(ts)
        else:
            ts = self._spaced(num_inference_steps)
            abar = self.alphas_cumprod[ts]
        self.num_inference_steps = num_inference_steps
        self._abar = np.append(abar, 1.0)                                 # abar_0 .. abar_{n-1}, then 1 behind the last timestep
        self._sigmas = np.sqrt((1.0 - self._abar) / self._abar)           # ... and sigma = 0 there
        self._step_index = 0
        self._build(ts)
        assert self._rows.shape == (len(self._eval_timesteps), PLAN_COLS)
        self.timesteps = torch.from_numpy(np.asarray(self._eval_timesteps, dtype=np.int64)).to(device)

    def _row(self, t, in_scale=1.0, m_x=0.0, m_eps=1.0, c_x=1.0, c0=0.0, c1=0.0, c2=0.0, c3=0.0, c_noise=0.0, push=0):
        return [float(t), in_scale, m_x, m_eps, c_x, c0, c1, c2, c3, c_noise, float(push), 0.0]

    def engine_plan(self):
        """[n_evals, 12] float64: timestep, in_scale, m_x, m_eps, c_x, c0, c1, c2, c3, c_noise, push, reserved -- per evaluation
        eps -> m0 = m_x x + m_eps eps;  x <- c_x x + c0 m0 + c1 h1 + c2 h2 + c3 h3 + c_noise noise;  push: (h1, h2, h3) <- (m0, h1, h2)."""
        self._need_chain()
        return self._rows.copy()

    def _need_chain(self):
        if self._rows is None:
            raise ValueError("call set_timesteps(num_inference_steps) first")

    # ------------------------------------------------------------------ diffusers interface
    @property
    def init_noise_sigma(self):
        return 1.0

    def scale_model_input(self, sample, timestep=None):
        """The model input of the CURRENT evaluation (the internal step index, not ``timestep``: Heun's timesteps repeat)."""
        self._need_chain()
        s = float(self._rows[min(self._step_index, len(self._rows) - 1), P_IN])
        return sample if s == 1.0 else sample * s

    def step(self, model_output, timestep, sample, generator=None, return_dict=True, noise=None):
        """One evaluation's update (``_update``: the class's published formula, host fp64 scalars as Python floats times the
        tensors); advances the internal step index that ``set_timesteps`` resets.  ``noise`` (not in diffusers): the draw of a
        stochastic step, given by the caller in place of ``generator``."""
        self._need_chain()
        if self._step_index >= len(self._rows):
            raise IndexError("step called more often than the chain has evaluations; call set_timesteps to start a new chain")
        self._given_noise = noise
        prev = self._update(self._step_index, model_output, sample, generator)
        self._step_index += 1
        return (prev,) if not return_dict else type("SchedulerOutput", (), {"prev_sample": prev})()


class EulerDiscreteScheduler(_LinearScheduler):
    """Euler steps of the probability-flow ODE in sigma (Karras et al. 2022, algorithm 1 without churn):
    x~' = x~ + (sigma_{i+1} - sigma_i) eps.  The same step as DDIM at eta = 0, written for x~ = x / sqrt(abar).
    Memory-derived, NOT pinned against diffusers."""

    @property
    def init_noise_sigma(self):
        return float((self._sigmas[0] ** 2 + 1.0) ** 0.5)

    def _build(self, ts):
        sg = self._sigmas
        self._eval_timesteps = list(ts)
        self._rows = np.array([self._row(t, in_scale=1.0 / (sg[i] ** 2 + 1.0) ** 0.5, c0=sg[i + 1] - sg[i]) for i, t in enumerate(ts)])

    def _update(self, i, eps, x, generator):
        return x + float(self._sigmas[i + 1] - self._sigmas[i]) * eps


class EulerAncestralDiscreteScheduler(EulerDiscreteScheduler):
    """Ancestral Euler (k-diffusion ``sample_euler_ancestral``): sigma_up = sqrt(sigma_{i+1}^2 (sigma_i^2 - sigma_{i+1}^2) / sigma_i^2),
    sigma_down = sqrt(sigma_{i+1}^2 - sigma_up^2), x~' = x~ + (sigma_down - sigma_i) eps + sigma_up n.  ``step`` draws n on EVERY step,
    the last (sigma_up = 0) included, so a chain always consumes num_inference_steps draws.  Memory-derived, NOT pinned against
    diffusers."""

    def _up_down(self, i):
        sg = self._sigmas
        up = (sg[i + 1] ** 2 * (sg[i] ** 2 - sg[i + 1] ** 2) / sg[i] ** 2) ** 0.5
        return float(up), float((sg[i + 1] ** 2 - up ** 2) ** 0.5)

    def _build(self, ts):
        sg = self._sigmas
        rows = []
        for i, t in enumerate(ts):
            up, down = self._up_down(i)
            rows.append(self._row(t, in_scale=1.0 / (sg[i] ** 2 + 1.0) ** 0.5, c0=down - sg[i], c_noise=up))
        self._eval_timesteps, self._rows = list(ts), np.array(rows)

    def _update(self, i, eps, x, generator):
        up, down = self._up_down(i)
        noise = self._given_noise if self._given_noise is not None else draw_noise(eps.shape, generator, eps.device, eps.dtype)
        return x + (down - float(self._sigmas[i])) * eps + up * noise


class HeunDiscreteScheduler(EulerDiscreteScheduler):
    """Heun's second-order method (Karras et al. 2022, algorithm 1): timesteps [t_0, t_1, t_1, ..., t_{n-1}, t_{n-1}], 2 n - 1
    evaluations.  Stage 1 at (t_i, sigma_i): x~_p = x~ + D eps_1, D = sigma_{i+1} - sigma_i; stage 2 at (t_{i+1}, sigma_{i+1}) on x~_p:
    x~' = x~ + D (eps_1 + eps_2) / 2, written on the current latents as x~_p + D/2 eps_2 - D/2 eps_1 (no saved sample); the last step
    (sigma_{i+1} = 0) is stage 1 only.  Memory-derived, NOT pinned against diffusers."""
    order = 2

    def _build(self, ts):
        sg = self._sigmas
        n = len(ts)
        rows, ets = [], []
        for i, t in enumerate(ts):
            d = sg[i + 1] - sg[i]
            rows.append(self._row(t, in_scale=1.0 / (sg[i] ** 2 + 1.0) ** 0.5, c0=d, push=1))
            ets.append(t)
            if i + 1 < n:
                rows.append(self._row(ts[i + 1], in_scale=1.0 / (sg[i + 1] ** 2 + 1.0) ** 0.5, c0=0.5 * d, c1=-0.5 * d))
                ets.append(ts[i + 1])
        self._eval_timesteps, self._rows = ets, np.array(rows)

    def _update(self, k, eps, x, generator):
        if k == 0:
            self._stage1 = None
        if self._stage1 is None:                                           # evaluations 0, 2, 4, ...: stage 1 of step k / 2
            i = k // 2
            d = float(self._sigmas[i + 1] - self._sigmas[i])
            if self._sigmas[i + 1] > 0.0:
                self._stage1 = (x, eps, d)
            return x + d * eps
        x0, eps1, d = self._stage1                                         # stage 2: from the saved sample
        self._stage1 = None
        return x0 + (0.5 * d) * (eps1 + eps)


class DPMSolverMultistepScheduler(_LinearScheduler):
    """DPM-Solver++ multistep (Lu et al. 2022), data prediction, ``solver_order`` 1 or 2 (2M, midpoint), ``lower_order_final``.
    alpha = sqrt(abar), sigma = sqrt(1 - abar), lambda = ln alpha - ln sigma, h = lambda_{i+1} - lambda_i, m = (x - sigma_i eps) / alpha_i;
    first order x' = (sigma_{i+1} / sigma_i) x - alpha_{i+1} expm1(-h) m_0; second order replaces m_0 by
    m_0 + (m_0 - m_1) / (2 r_0), r_0 = (lambda_i - lambda_{i-1}) / h.  First order on the first step and on the last step, which lands on
    sigma = 0 (x' = m_0) whatever n is -- so ``lower_order_final`` (first order on the last step of a short chain) changes nothing
    here; it is accepted for interface compatibility only, and ``lower_order_final=False`` is refused because the second-order
    formula does not exist at h = inf.  Memory-derived, NOT pinned against diffusers."""

    def __init__(self, solver_order=2, lower_order_final=True, algorithm_type="dpmsolver++", solver_type="midpoint", **kw):
        if solver_order not in (1, 2) or algorithm_type != "dpmsolver++" or solver_type != "midpoint":
            raise ValueError("DPMSolverMultistepScheduler: dpmsolver++ with the midpoint solver at solver_order 1 or 2 only")
        if not lower_order_final:
            raise ValueError("DPMSolverMultistepScheduler: the last step lands on sigma = 0 and is always first order; "
                             "lower_order_final=False cannot be honoured")
        self.solver_order, self.lower_order_final = solver_order, True
        super().__init__(**kw)

    def _build(self, ts):
        ab = self._abar
        n = len(ts)
        al, sg = np.sqrt(ab), np.sqrt(1.0 - ab)
        with np.errstate(divide="ignore"):
            lam = np.log(al) - np.log(sg)                                  # +inf behind the last timestep
        rows = []
        for i, t in enumerate(ts):
            kw = dict(m_x=1.0 / al[i], m_eps=-sg[i] / al[i], push=1)
            if i + 1 == n:                                                 # lands on sigma = 0: sigma'/sigma = 0, -alpha' expm1(-inf) = 1
                rows.append(self._row(t, c_x=0.0, c0=1.0, **kw))
                continue
            h = lam[i + 1] - lam[i]
            a = -al[i + 1] * np.expm1(-h)
            first = self.solver_order == 1 or i == 0                       # (the last step is the branch above whatever n is)
            if first:
                rows.append(self._row(t, c_x=sg[i + 1] / sg[i], c0=a, **kw))
            else:
                r0 = (lam[i] - lam[i - 1]) / h
                rows.append(self._row(t, c_x=sg[i + 1] / sg[i], c0=a * (1.0 + 0.5 / r0), c1=-a * 0.5 / r0, **kw))
        self._eval_timesteps, self._rows = list(ts), np.array(rows)
        self._al, self._sg, self._lam = al, sg, lam

    def _update(self, i, eps, x, generator):
        al, sg, lam = self._al, self._sg, self._lam
        m0 = (x - float(sg[i]) * eps) / float(al[i])
        m1, self._m_prev = (None if i == 0 else self._m_prev), m0
        if i + 1 == len(self._rows):
            return m0
        h = lam[i + 1] - lam[i]
        if not (self.solver_order == 1 or i == 0):
            r0 = (lam[i] - lam[i - 1]) / h
            m0 = m0 + float(0.5 / r0) * (m0 - m1)
        return float(sg[i + 1] / sg[i]) * x - float(al[i + 1] * np.expm1(-h)) * m0


class DDIMInverseScheduler(_LinearScheduler):
    """DDIM inversion for text-to-video: the algebraic inverse of this project's ``DDIMScheduler`` chain at eta = 0, with its
    constructor keys (``set_alpha_to_one`` among them).  ``set_timesteps(n)`` gives the sampling set of ``n`` steps in ASCENDING
    order u_0 < ... < u_{n-1}.  Evaluation j runs the denoiser at u_j and carries x from level a_from to level a_to = abar[u_j], where
    a_from = ``final_alpha_cumprod`` (1, or abar[0] with ``set_alpha_to_one=False``) for j = 0 and abar[u_{j-1}] after it:

        x' = sqrt(a_to / a_from) x + (sqrt(1 - a_to) - sqrt(a_to (1 - a_from) / a_from)) eps

    which undoes the DDIM step from a_to down to a_from for the same eps.  After n evaluations x is at level abar[u_{n-1}], where a
    DDIM run of the same n starts.  One ``engine_plan()`` row per evaluation (m_eps = 1, c_x, c0; no history, no noise), so
    ``latte_t2v_guided_linear_loop`` runs the chain unchanged.

    Memory-derived and NOT pinned against diffusers.  The denoiser sees the timestep of the level being ENTERED (u_j with x still at
    the level below it) -- the convention of diffusers-style inversion; the class-conditional engine's ``ddim_reverse_sample`` follows the
    reference instead and evaluates at the level being LEFT."""

    def __init__(self, set_alpha_to_one=True, clip_sample=False, **kw):
        if clip_sample:
            raise ValueError("DDIMInverseScheduler has no clip_sample: a clamped x_0 prediction has no inverse")
        super().__init__(**kw)
        self.final_alpha_cumprod = 1.0 if set_alpha_to_one else float(self.alphas_cumprod[0])

    def _build(self, ts):
        up = [int(t) for t in ts[::-1]]                                    # ascending
        self._eval_timesteps = up
        rows, a_from = [], self.final_alpha_cumprod
        for t, a_to in zip(up, self._abar[-2::-1].tolist()):               # abar at the set's timesteps, ascending too
            rows.append(self._row(t, c_x=(a_to / a_from) ** 0.5, c0=(1.0 - a_to) ** 0.5 - (a_to * (1.0 - a_from) / a_from) ** 0.5))
            a_from = a_to
        self._rows = np.array(rows)

    def _update(self, i, eps, x, generator):
        return float(self._rows[i, P_CX]) * x + float(self._rows[i, P_C0]) * eps
