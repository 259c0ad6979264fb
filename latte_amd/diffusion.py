"""Host-side mirror of the reference sampler interface (``diffusion/__init__.py``, ``respace.py``,
``gaussian_diffusion.py``) on top of the C-ABI.

* schedules: ``latte_schedule_*`` (host fp64, bit-exact timestep maps);
* per-step update: ``latte_sampler_step`` (one fused HIP kernel instead of ~25 elementwise ops and
  8-12 host->device coefficient copies per step, gaussian_diffusion.py:869-881);
* whole loop: when the model callable is a ``latte_amd.Latte`` method the loop runs inside the
  engine (``latte_sample_loop``; ``latte_invert_loop`` for DDIM inversion); any other callable following
  the model-callable protocol is driven step by step with the same update kernel;
* ``linear_sample_loop`` (not in the reference): Euler, Euler-ancestral, Heun and DPM-Solver++(2M) on the diffusion's own
  timesteps, as ONE ``latte_sample_plan_loop`` call for a ``latte_amd.Latte`` method;
* ``known_sample_loop`` (not in the reference): DDIM / DDPM with part of the clip held fixed (prediction, interpolation, inpainting by
  replacement), as ``latte_sample_loop_known`` calls for a ``latte_amd.Latte`` method;
* ``window_sample_loop`` (not in the reference): clips longer than ``num_frames`` by overlapping temporal windows, as
  ``latte_sample_loop_windows`` / ``latte_sample_plan_loop_windows`` calls for a ``latte_amd.Latte`` method.
"""
import ctypes
from types import SimpleNamespace

import numpy as np
import torch

from . import _lib
from ._lib import LatteError, check, load_library, ptr, stream_ptr
from .known import known_blend, level_coefs
from .windows import repeat_per_window, window_gather, window_merge, window_starts
from .models import Latte
from .schedulers import (DPMSolverMultistepScheduler, EulerAncestralDiscreteScheduler, EulerDiscreteScheduler,
                         HeunDiscreteScheduler)

_TABLES = ["betas", "alphas_cumprod", "alphas_cumprod_prev", "alphas_cumprod_next", "sqrt_recip_alphas_cumprod",
           "sqrt_recipm1_alphas_cumprod", "posterior_variance", "posterior_log_variance_clipped",
           "posterior_mean_coef1", "posterior_mean_coef2", "log_betas", "sqrt_alphas_cumprod",
           "sqrt_one_minus_alphas_cumprod"]
_LOSS = {"mse": 0, "rescaled_mse": 1, "kl": 2, "rescaled_kl": 3}
_METHOD = {"ddpm": 0, "ddim": 1, "ddim_reverse": 2}
LINEAR_METHODS = {"euler": EulerDiscreteScheduler, "euler_a": EulerAncestralDiscreteScheduler, "heun": HeunDiscreteScheduler,
                  "dpmsolver++": DPMSolverMultistepScheduler}


class SpacedDiffusion:
    """Stand-in for ``respace.SpacedDiffusion`` as built by ``create_diffusion`` (diffusion/__init__.py:32-46):
    EPSILON or START_X mean type, LEARNED_RANGE / FIXED_LARGE / FIXED_SMALL variance."""

    SEGMENT_BYTES = 256 << 20   # per-step noise / trail buffers of one fused-loop segment (see _loop)

    def __init__(self, timestep_respacing, noise_schedule="linear", diffusion_steps=1000, predict_xstart=False,
                 learn_sigma=True, sigma_small=False, loss_type="mse"):
        if loss_type not in _LOSS:
            raise LatteError(f"loss_type must be one of {sorted(_LOSS)}")
        self.loss_type = loss_type
        lib = load_library()
        h = _lib.c_void()
        if isinstance(timestep_respacing, (list, tuple)):
            timestep_respacing = ",".join(str(int(v)) for v in timestep_respacing)
        spec = "" if timestep_respacing is None else str(timestep_respacing)
        check(lib.latte_schedule_create(int(diffusion_steps), spec.encode(), noise_schedule.encode(), h))
        self._h = h
        check(lib.latte_schedule_set_model_types(h, int(bool(predict_xstart)), int(bool(learn_sigma)), int(bool(sigma_small))))
        self.predict_xstart, self.learn_sigma, self.sigma_small = bool(predict_xstart), bool(learn_sigma), bool(sigma_small)
        self.original_num_steps = int(diffusion_steps)
        self.num_timesteps = lib.latte_schedule_num_timesteps(h)
        n = self.num_timesteps
        tm = np.empty(n, dtype=np.int64)
        check(lib.latte_schedule_timestep_map(h, tm.ctypes.data_as(ctypes.c_void_p), n))
        self.timestep_map = tm.tolist()
        self.use_timesteps = set(self.timestep_map)
        for name in _TABLES:
            if name == "posterior_log_variance_clipped" and n < 2:
                setattr(self, name, np.array([]))
                continue
            arr = np.empty(n, dtype=np.float64)
            check(lib.latte_schedule_table(h, name.encode(), arr.ctypes.data_as(ctypes.c_void_p), n))
            setattr(self, name, arr)

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                load_library().latte_schedule_destroy(self._h)
        except Exception:
            pass

    # ------------------------------------------------------------------ helpers
    @staticmethod
    def _engine_model(model):
        """(Latte instance, uses_cfg) when `model` is a bound latte_amd.Latte method, else (None, False)."""
        owner = getattr(model, "__self__", None)
        if isinstance(model, Latte):
            return model, False
        if isinstance(owner, Latte):
            fn = getattr(model, "__func__", None)
            if fn is Latte.forward:
                return owner, False
            if fn is Latte.forward_with_cfg:
                return owner, True
        return None, False

    def _engine_chain(self, model, img, model_kwargs, hooks=False, windows=None):
        """The engine path of a loop: None unless `model` is a bound latte_amd.Latte method called with kwargs the engine knows and no
        hooks; else what its chain calls take -- eng, x32 (`img` on the model's device, sampled in place), y64, B, uses_cfg, cfg_scale --
        with the text embedding installed.  ``windows`` (window_sample_loop): `img` is a long clip, the engine holds B * windows clips
        and the text embedding is installed per clip."""
        owner, uses_cfg = self._engine_model(model)
        if owner is None or hooks or not set(model_kwargs) <= {"y", "use_fp16", "cfg_scale", "text_embedding"}:
            return None
        _lib.require_gpu()
        B = img.shape[0]
        x32, _, y64 = owner._prep(img, torch.zeros(B, dtype=torch.int64), model_kwargs.get("y"),
                                   frames=None if windows is None else img.shape[1])
        windows = windows or 1
        cfg_scale = float(model_kwargs.get("cfg_scale", 7.0)) if uses_cfg else 1.0
        eng = owner.engine(B * windows, guided=uses_cfg)
        te = model_kwargs.get("text_embedding")
        owner._set_text(te if te is None or windows == 1 else te.repeat_interleave(windows, dim=0), B * windows, guided=uses_cfg)
        return SimpleNamespace(eng=eng, x32=x32, y64=y64, B=B, uses_cfg=int(uses_cfg), cfg_scale=cfg_scale)

    @staticmethod
    def _segments(start, end, seg):
        """Inclusive (first, last) index segments of at most `seg` indices from `start` to `end`, descending when end < start."""
        step = -1 if end < start else 1
        i = start
        while (end - i) * step >= 0:
            last = i + step * min(seg - 1, (end - i) * step)
            yield i, last
            i = last + step

    def _engine_run(self, ec, start, end, seg, progressive, call, x0_trail=True):
        """The chain of `ec` over the indices start ... end, one engine call per segment: ``call(first, last, trail_sample, trail_x0)``
        (trail pointers, NULL unless progressive) makes it and returns the noise it fed, or None.  Only ONE segment's noise and trails
        exist at a time.  Yields {"sample", "pred_xstart"} per index when progressive, else the final sample once."""
        x32 = ec.x32
        for first, last in self._segments(start, end, seg):
            cnt = abs(last - first) + 1
            trail_s = trail_0 = None
            if progressive:
                trail_s = torch.empty((cnt,) + tuple(x32.shape), device=x32.device, dtype=torch.float32)
                trail_0 = torch.empty_like(trail_s) if x0_trail else None
            with torch.cuda.device(x32.device):
                nz = call(first, last, ptr(trail_s), ptr(trail_0))
                if nz is not None or progressive:
                    torch.cuda.current_stream().synchronize()      # the segment's buffers are released / handed out next
            for k in range(cnt if progressive else 0):
                yield {"sample": trail_s[k], "pred_xstart": None if trail_0 is None else trail_0[k]}
        if not progressive:
            yield {"sample": x32, "pred_xstart": None}

    @staticmethod
    def _progress(seq, progress):
        if progress:
            from tqdm.auto import tqdm
            return tqdm(seq)
        return seq

    @staticmethod
    def _last_sample(loop):
        """Runs a progressive generator to its last item -> that item's sample."""
        final = None
        for final in loop:
            pass
        return final["sample"]

    def _device(self, model, device, fallback=None):
        """`fallback`: the tensor whose device a callable that is no latte_amd.Latte method runs on."""
        if device is not None:
            return torch.device(device)
        if fallback is not None and self._engine_model(model)[0] is None:
            return fallback.device
        owner = getattr(model, "__self__", model)
        return next(owner.parameters()).device                                     # gd:487-488

    def _step(self, method, model_output, x, index, noise, eta, clip_denoised, denoised_fn=None, cond_fn=None,
              model_kwargs=None):
        """p_mean_variance + p_sample / ddim_sample / ddim_reverse_sample of one step on the engine (gd:254-336, :380-421,
        :517-602), with the two caller hooks: ``denoised_fn`` on the x_start prediction before the clamp (gd:316-321) and
        ``cond_fn(x, t)`` with ORIGINAL timesteps (rs:100-104; condition_mean for DDPM, condition_score for DDIM and its
        reverse)."""
        _lib.require_gpu()
        B, F, C = x.shape[:3]
        want = (B, F, C * 2 if self.learn_sigma else C, *x.shape[3:])              # gd:290 / :338
        if model_output.shape != want:
            raise AssertionError(f"model output shape {tuple(model_output.shape)} != {want}")
        x32 = x.float().contiguous()
        mo = model_output.float().contiguous()
        nz = None if noise is None else noise.float().contiguous()
        sample = torch.empty_like(x32)
        x0 = torch.empty_like(x32)
        hw = int(np.prod(x.shape[3:]))
        lib = load_library()
        args = (self._h, _METHOD[method], int(index), float(eta), int(bool(clip_denoised)), ptr(x32), ptr(mo), ptr(nz))
        x0_in = grad = None
        with torch.cuda.device(x32.device):
            if denoised_fn is not None:
                check(lib.latte_sampler_step_ex(*args, None, None, 1, B, F, C, hw, None, ptr(x0), stream_ptr()))
                x0_in = denoised_fn(x0).float().contiguous()
                if x0_in.shape != x32.shape:
                    raise AssertionError("denoised_fn must keep the shape of its argument")
            if cond_fn is not None:
                t = torch.full((B,), self.timestep_map[index], device=x32.device, dtype=torch.int64)
                grad = cond_fn(x, t, **(model_kwargs or {})).float().contiguous()
                if grad.shape != x32.shape:
                    raise AssertionError("cond_fn must return a gradient of x's shape")
            check(lib.latte_sampler_step_ex(*args, ptr(x0_in), ptr(grad), 0, B, F, C, hw, ptr(sample), ptr(x0), stream_ptr()))
        return {"sample": sample, "pred_xstart": x0}

    def _call_model(self, model, x, index, model_kwargs):
        # respace.py:125-130: the model sees ORIGINAL timesteps
        t = torch.full((x.shape[0],), self.timestep_map[index], device=x.device, dtype=torch.int64)
        out = model(x, t, **model_kwargs)
        if isinstance(out, tuple):                                                  # gd:284-287
            out = out[0]
        return out

    # ------------------------------------------------------------------ single steps (gd:380-421, :517-564)
    def p_sample(self, model, x, t, clip_denoised=True, denoised_fn=None, cond_fn=None, model_kwargs=None):
        index = self._uniform_index(t)
        out = self._call_model(model, x, index, model_kwargs or {})
        return self._step("ddpm", out, x, index, torch.randn_like(x.float()), 0.0, clip_denoised, denoised_fn, cond_fn,
                          model_kwargs)

    def ddim_sample(self, model, x, t, clip_denoised=True, denoised_fn=None, cond_fn=None, model_kwargs=None, eta=0.0):
        index = self._uniform_index(t)
        out = self._call_model(model, x, index, model_kwargs or {})
        return self._step("ddim", out, x, index, torch.randn_like(x.float()), eta, clip_denoised, denoised_fn, cond_fn,
                          model_kwargs)

    def ddim_reverse_sample(self, model, x, t, clip_denoised=True, denoised_fn=None, cond_fn=None, model_kwargs=None, eta=0.0):
        """``GaussianDiffusion.ddim_reverse_sample`` (gd:566-602): the deterministic DDIM step from level ``t`` UP to level
        ``t + 1`` -> {"sample", "pred_xstart"}.  One timestep index shared by the batch, as ``_vb_terms_bpd`` takes it."""
        assert eta == 0.0, "Reverse ODE only for deterministic path"                  # gd:580
        index = self._uniform_index(t)
        out = self._call_model(model, x, index, model_kwargs or {})
        return self._step("ddim_reverse", out, x, index, None, 0.0, clip_denoised, denoised_fn, cond_fn, model_kwargs)

    @staticmethod
    def _uniform_index(t):
        tv = t.tolist()
        if any(v != tv[0] for v in tv):
            raise LatteError("the fused sampler step takes one timestep index for the whole batch "
                             "(the sampling loops always do, gaussian_diffusion.py:503,671)")
        return int(tv[0])

    # ------------------------------------------------------------------ loops (gd:423-515, :604-684)
    def _index_range(self, start_index, end_index, ascending):
        """The inclusive respaced index range of a partial chain; None = the end of the full chain on that side."""
        n = self.num_timesteps
        first, last = (0, n - 1) if ascending else (n - 1, 0)
        start = first if start_index is None else int(start_index)
        end = last if end_index is None else int(end_index)
        lo, hi = (start, end) if ascending else (end, start)
        if not 0 <= lo <= hi < n:
            raise LatteError(f"bad index range {start} ... {end} for {n} timesteps")
        return start, end

    def _loop(self, method, model, shape, noise, clip_denoised, denoised_fn, cond_fn, model_kwargs, device, progress,
              eta, progressive, start_index=None, end_index=None):
        _lib.require_gpu()
        start, end = self._index_range(start_index, end_index, ascending=False)
        model_kwargs = dict(model_kwargs or {})
        device = self._device(model, device)
        assert isinstance(shape, (tuple, list))
        img = noise if noise is not None else torch.randn(*shape, device=device)
        img = img.to(device=device, dtype=torch.float32).contiguous().clone()
        n = self.num_timesteps
        needs_noise = method == "ddpm" or eta != 0.0
        ec = self._engine_chain(model, img, model_kwargs, denoised_fn is not None or cond_fn is not None)
        if ec is not None:
            # ---- whole chain inside the engine
            # The chain runs in segments of consecutive steps so that the per-step noise (and the progressive trails) of
            # only ONE segment exist at a time: 65 MB per 250-step sample-chain otherwise, 4.2 GB at B = 64.  The draws
            # are the reference's -- one torch.randn_like per step, in step order (gd:413,555) -- whatever the split.
            seg = max(1, min(n, self.SEGMENT_BYTES // max(ec.x32.numel() * 4, 1)))
            lib = load_library()

            def call(i, lo, trail_s, trail_0):
                nz = torch.stack([torch.randn_like(ec.x32) for _ in range(i - lo + 1)]) if needs_noise else None
                check(lib.latte_sample_loop_ex(ec.eng, self._h, _METHOD[method], float(eta), int(bool(clip_denoised)), ec.uses_cfg,
                                               ec.cfg_scale, ptr(ec.x32), ptr(ec.y64), ec.B, i, lo, ptr(nz), trail_s, trail_0,
                                               stream_ptr()))
                return nz

            yield from self._engine_run(ec, start, end, seg, progressive, call)
            return
        # ---- generic model callable, step by step
        for i in self._progress(list(range(end, start + 1))[::-1], progress):
            out = self._call_model(model, img, i, model_kwargs)
            nz = torch.randn_like(img) if needs_noise else None
            r = self._step(method, out, img, i, nz, eta, clip_denoised, denoised_fn, cond_fn, model_kwargs)
            yield r
            img = r["sample"]

    def p_sample_loop_progressive(self, model, shape, noise=None, clip_denoised=True, denoised_fn=None, cond_fn=None,
                                  model_kwargs=None, device=None, progress=False):
        yield from self._loop("ddpm", model, shape, noise, clip_denoised, denoised_fn, cond_fn, model_kwargs, device,
                              progress, 0.0, True)

    def ddim_sample_loop_progressive(self, model, shape, noise=None, clip_denoised=True, denoised_fn=None,
                                     cond_fn=None, model_kwargs=None, device=None, progress=False, eta=0.0):
        yield from self._loop("ddim", model, shape, noise, clip_denoised, denoised_fn, cond_fn, model_kwargs, device,
                              progress, eta, True)

    def p_sample_loop(self, model, shape, noise=None, clip_denoised=True, denoised_fn=None, cond_fn=None,
                      model_kwargs=None, device=None, progress=False):
        return self._last_sample(self._loop("ddpm", model, shape, noise, clip_denoised, denoised_fn, cond_fn, model_kwargs, device,
                                            progress, 0.0, False))

    def ddim_sample_loop(self, model, shape, noise=None, clip_denoised=True, denoised_fn=None, cond_fn=None,
                         model_kwargs=None, device=None, progress=False, eta=0.0, start_index=None, end_index=None):
        """``GaussianDiffusion.ddim_sample_loop`` (gd:604-635).  ``start_index`` / ``end_index`` (not in the reference; default
        the full chain T-1 ... 0) run the respaced steps start ... end descending on ``noise`` taken as level ``start``: the
        way back from a ``ddim_reverse_sample_loop`` that ended at ``end_index = start - 1``."""
        return self._last_sample(self._loop("ddim", model, shape, noise, clip_denoised, denoised_fn, cond_fn, model_kwargs, device,
                                            progress, eta, False, start_index, end_index))

    # ------------------------------------------------------------------ linear samplers (not in the reference)
    def linear_scheduler(self, method="dpmsolver++"):
        """The ``latte_amd.schedulers`` object of ``method`` ("euler" | "euler_a" | "heun" | "dpmsolver++") set to THIS diffusion's
        timesteps: ``timestep_map`` descending with ``alphas_cumprod`` at them, so ``create_diffusion("20")`` means 20 steps (39
        evaluations for Heun) as it does for ``ddim_sample_loop``.  Host only."""
        if self.predict_xstart:
            raise LatteError("linear_sample_loop: the linear samplers take an eps-prediction model (predict_xstart=False)")
        if method not in LINEAR_METHODS:
            raise LatteError(f"linear_sample_loop: method must be one of {sorted(LINEAR_METHODS)}, got {method!r}")
        sch = LINEAR_METHODS[method](num_train_timesteps=self.original_num_steps)
        sch.set_timesteps(timesteps=self.timestep_map[::-1], alphas_cumprod_at=self.alphas_cumprod[::-1])
        return sch

    def _linear_loop(self, model, shape, noise, method, model_kwargs, device, progress, step_noise, progressive):
        sch = self.linear_scheduler(method)
        plan = np.ascontiguousarray(sch.engine_plan(), dtype=np.float64)
        n_evals = plan.shape[0]
        model_kwargs = dict(model_kwargs or {})
        assert isinstance(shape, (tuple, list))
        device = self._device(model, device, noise)
        img = noise if noise is not None else torch.randn(*shape, device=device)
        img = img.to(device=device, dtype=torch.float32).contiguous() * float(sch.init_noise_sigma)
        if img.dim() != 5:
            raise LatteError("shape must be [N, F, C, H, W]")
        nz = None
        if step_noise is not None:
            if tuple(step_noise.shape) != (n_evals,) + tuple(img.shape):
                raise LatteError(f"step_noise must be [{n_evals}, ...latents]: one slab per denoiser evaluation of {method!r}")
            nz = step_noise.to(device=device, dtype=torch.float32).contiguous()
        ec = self._engine_chain(model, img, model_kwargs)
        if ec is not None:
            # ---- whole chain inside the engine: one call, one trail
            lib = load_library()
            check(lib.latte_engine_set_option(ec.eng, b"train_timesteps", self.original_num_steps))

            def call(first, last, trail, _):
                check(lib.latte_sample_plan_loop(ec.eng, ec.uses_cfg, ec.cfg_scale, ptr(ec.x32), ptr(ec.y64), ec.B, n_evals,
                                                 plan.ctypes.data, ptr(nz), trail, stream_ptr()))
                return nz

            yield from self._engine_run(ec, 0, n_evals - 1, n_evals, progressive, call, x0_trail=False)
            return
        # ---- generic model callable, step by step: the scheduler's own scale_model_input / step around it
        C = img.shape[2]
        for k, t in self._progress(list(enumerate(sch.timesteps.tolist())), progress):
            tt = torch.full((img.shape[0],), t, device=img.device, dtype=torch.int64)   # ORIGINAL timesteps: no _WrappedModel here
            out = model(sch.scale_model_input(img, t), tt, **model_kwargs)
            if isinstance(out, tuple):
                out = out[0]
            if out.shape[2] not in (C, 2 * C):
                raise AssertionError(f"model output has {out.shape[2]} channels for {C}-channel latents")
            eps = out[:, :, :C].float()                            # the learned-sigma half is dropped; forward_with_cfg already guided it
            img = sch.step(eps, t, img, return_dict=False, noise=None if nz is None else nz[k])[0]
            yield {"sample": img, "pred_xstart": None}

    @staticmethod
    def _no_known(known, known_mask):
        if known is not None or known_mask is not None:
            raise LatteError("linear_sample_loop: no known-region sampling with the linear samplers -- their samples live at other noise "
                             "levels (sigma-scaled) and Heun has intermediate states; use known_sample_loop (DDIM / DDPM)")

    def linear_sample_loop_progressive(self, model, shape, noise=None, method="dpmsolver++", model_kwargs=None, device=None,
                                       progress=False, step_noise=None, known=None, known_mask=None):
        """``linear_sample_loop`` yielding {"sample", "pred_xstart": None} after every denoiser evaluation."""
        self._no_known(known, known_mask)
        yield from self._linear_loop(model, shape, noise, method, model_kwargs, device, progress, step_noise, True)

    def linear_sample_loop(self, model, shape, noise=None, method="dpmsolver++", model_kwargs=None, device=None, progress=False,
                           step_noise=None, known=None, known_mask=None):
        """Sampling with a linear multistep / Runge-Kutta sampler in place of DDIM / DDPM: ``method`` "euler", "euler_a" (ancestral),
        "heun" or "dpmsolver++" (2M) from ``latte_amd.schedulers``, on this diffusion's own ``timestep_map`` (``linear_scheduler``).  The
        initial latents are ``noise * init_noise_sigma``; the model sees ORIGINAL timesteps; the learned-sigma half of its output is
        dropped and nothing is clipped.  With ``model.forward`` / ``model.forward_with_cfg`` of a ``latte_amd.Latte`` and known kwargs
        the chain is ONE ``latte_sample_plan_loop`` call; any other callable is driven through the scheduler's ``scale_model_input`` /
        ``step``.  ``step_noise`` [n_evals, ...latents] gives the draws of the stochastic steps ("euler_a") to either path; without it
        the engine path draws from the engine's Philox stream (option "seed"), the step-by-step path from ``torch.randn``.  Run over the
        same timesteps, "euler" is ``ddim_sample_loop(eta=0, clip_denoised=False)``.  No hooks (``denoised_fn`` / ``cond_fn``), and no
        known-region sampling: ``known`` / ``known_mask`` raise (``known_sample_loop`` serves DDIM / DDPM)."""
        self._no_known(known, known_mask)
        return self._last_sample(self._linear_loop(model, shape, noise, method, model_kwargs, device, progress, step_noise, False))

    # ------------------------------------------------------------------ known-region sampling (not in the reference)
    def known_chain_slabs(self, method="ddim", eta=0.0, resample=1, start_index=None, end_index=None, blend_start=True):
        """The number of noise slabs (each of the latents' size) a known-region chain consumes: ``latte_known_chain_slabs``, the one
        definition of the count and the order -- the start blend; then per repetition the step's own noise (DDPM at i > 0, DDIM where
        sigma != 0), the blend's (i > 0), the forward jump's.  Host only."""
        if method not in ("ddim", "ddpm"):
            raise LatteError(f"known_sample_loop: method must be 'ddim' or 'ddpm', got {method!r}")
        start, end = self._index_range(start_index, end_index, ascending=False)
        n = _lib.c_i64(0)
        check(load_library().latte_known_chain_slabs(self._h, _METHOD[method], float(eta), start, end, int(resample), int(bool(blend_start)),
                                                     ctypes.byref(n)))
        return int(n.value)

    def _known_loop(self, method, model, shape, known, known_mask, noise, clip_denoised, denoised_fn, cond_fn, model_kwargs, device,
                    progress, eta, resample, start_index, end_index, chain_noise, blend_start, progressive):
        resample = int(resample)
        n_slabs = self.known_chain_slabs(method, eta, resample, start_index, end_index, blend_start)   # refuses resample < 1 too
        _lib.require_gpu()
        start, end = self._index_range(start_index, end_index, ascending=False)
        model_kwargs = dict(model_kwargs or {})
        device = self._device(model, device, noise if noise is not None else known)   # a plain callable: the start, else the known clip
        assert isinstance(shape, (tuple, list))
        img = noise if noise is not None else torch.randn(*shape, device=device)
        img = img.to(device=device, dtype=torch.float32).contiguous().clone()
        if img.dim() != 5:
            raise LatteError("shape must be [N, F, C, H, W]")
        B, F, C, H, W = img.shape
        if (H * W) % 4:
            raise LatteError("known_sample_loop: H * W must be a multiple of 4 (16-byte accesses of the blend kernel)")
        kn = known.to(device=device, dtype=torch.float32)
        mk = known_mask.to(device=device, dtype=torch.float32)
        if kn.shape[0] * 2 == B:                                    # the doubled batch of forward_with_cfg: double them as z is doubled
            kn = torch.cat([kn, kn])
        if mk.shape[0] * 2 == B:
            mk = torch.cat([mk, mk])
        kn, mk = kn.contiguous(), mk.contiguous()
        if kn.shape != img.shape:
            raise LatteError(f"known_sample_loop: known must be {tuple(img.shape)}, got {tuple(kn.shape)}")
        if tuple(mk.shape) != (B, F, H, W):
            raise LatteError(f"known_sample_loop: known_mask must be [N, F, H, W] = {(B, F, H, W)}, got {tuple(mk.shape)}")
        slabs = None
        if chain_noise is not None:
            if tuple(chain_noise.shape) != (n_slabs,) + tuple(img.shape):
                raise LatteError(f"chain_noise must be [{n_slabs}, ...latents]: one slab per draw of the chain (known_chain_slabs)")
            slabs = chain_noise.to(device=device, dtype=torch.float32).contiguous()
        taken = 0

        def take(cnt):   # the next cnt slabs: the caller's, else one torch.randn_like each, in slab order
            nonlocal taken
            taken += cnt
            if cnt == 0:
                return None
            return slabs[taken - cnt:taken] if slabs is not None else torch.stack([torch.randn_like(img) for _ in range(cnt)])

        ec = self._engine_chain(model, img, model_kwargs, denoised_fn is not None or cond_fn is not None)
        if ec is not None:
            # ---- whole chain inside the engine, in segments of consecutive indices as _loop segments its noise
            seg = max(1, min(self.num_timesteps, self.SEGMENT_BYTES // max(ec.x32.numel() * 4 * 3 * resample, 1)))
            lib = load_library()

            def call(i, lo, trail_s, trail_0):
                first = int(bool(blend_start) and i == start)
                nz = take(self.known_chain_slabs(method, eta, resample, i, lo, first))
                check(lib.latte_sample_loop_known(ec.eng, self._h, _METHOD[method], float(eta), int(bool(clip_denoised)), ec.uses_cfg,
                                                  ec.cfg_scale, ptr(ec.x32), ptr(ec.y64), B, i, lo, ptr(kn), ptr(mk), resample, first,
                                                  ptr(nz), trail_s, trail_0, stream_ptr()))
                return nz

            yield from self._engine_run(ec, start, end, seg, progressive, call)
            assert taken == n_slabs
            return
        # ---- generic model callable, step by step: _step, then latte_known_blend, then the jump
        def blend(x, abar, draws):
            a, b = level_coefs(abar) if draws else (1.0, 0.0)
            z = take(1) if draws else None
            return known_blend(x, kn, mk, a, b, None if z is None else z[0])

        if blend_start:
            img = blend(img, self.alphas_cumprod[start], True)
        for i in self._progress(list(range(end, start + 1))[::-1], progress):
            # the step's own draws: what the one-index chain takes besides its blend
            step_draws = self.known_chain_slabs(method, eta, 1, i, i, False) - int(i > 0)
            for u in range(1, resample + 1):
                out = self._call_model(model, img, i, model_kwargs)
                z = take(step_draws)
                r = self._step(method, out, img, i, None if z is None else z[0], eta, clip_denoised, denoised_fn, cond_fn, model_kwargs)
                img = blend(r["sample"], self.alphas_cumprod_prev[i], i > 0)
                if u < resample and i > 0:                           # back to level i (RePaint's resampling)
                    beta = np.float32(self.betas[i])
                    img = float(np.sqrt(np.float32(1.0) - beta)) * img + float(np.sqrt(beta)) * take(1)[0]
            yield {"sample": img, "pred_xstart": r["pred_xstart"]}
        assert taken == n_slabs

    def known_sample_loop_progressive(self, model, shape, known, known_mask, method="ddim", noise=None, clip_denoised=True,
                                      model_kwargs=None, eta=0.0, resample=1, start_index=None, end_index=None, chain_noise=None,
                                      device=None, progress=False, denoised_fn=None, cond_fn=None, blend_start=True):
        """``known_sample_loop`` yielding {"sample", "pred_xstart"} after every respaced index (after the blend of its last
        repetition)."""
        yield from self._known_loop(method, model, shape, known, known_mask, noise, clip_denoised, denoised_fn, cond_fn, model_kwargs,
                                    device, progress, eta, resample, start_index, end_index, chain_noise, blend_start, True)

    def known_sample_loop(self, model, shape, known, known_mask, method="ddim", noise=None, clip_denoised=True, model_kwargs=None,
                          eta=0.0, resample=1, start_index=None, end_index=None, chain_noise=None, device=None, progress=False,
                          denoised_fn=None, cond_fn=None, blend_start=True):
        """Sampling with part of the clip held fixed -- animate a first frame, continue a clip, fill between key frames, repaint a
        region -- by the replacement scheme of Video Diffusion Models / RePaint, on unchanged weights (not in the reference).  ``known``
        [N, F, C, H, W]: the clean latents of the known clip; ``known_mask`` [N, F, H, W] (``latte_amd.known_mask``): 1 = known, 0 =
        generated.  The chain is ``p_sample_loop`` / ``ddim_sample_loop`` (``method``) over ``start_index`` ... ``end_index``; before
        the first step (``blend_start``) and after every step the known part of the sample is overwritten with ``known`` diffused to
        the level the sample is at -- ``alphas_cumprod_prev[i]`` after index i, so the known part of the result is ``known`` bit for
        bit.  ``resample`` > 1 repeats every index that many times with the one-level forward jump ``sqrt(1 - beta_i) x + sqrt(beta_i)
        z`` between repetitions, which lets the generated part agree with the known part.  With ``forward_with_cfg`` on the doubled
        batch, ``known`` / ``known_mask`` of half the batch are doubled as ``z`` is.
        With ``model.forward`` / ``model.forward_with_cfg`` of a ``latte_amd.Latte``, known kwargs and no hooks the chain is ONE
        ``latte_sample_loop_known`` call per segment; any other callable goes step by step through the step kernel and
        ``latte_known_blend``.  ``chain_noise`` [known_chain_slabs(...), ...latents] gives every draw to either path, in slab order;
        without it each slab is one ``torch.randn_like``.  The linear samplers have no known-region form (``linear_sample_loop``)."""
        return self._last_sample(self._known_loop(method, model, shape, known, known_mask, noise, clip_denoised, denoised_fn, cond_fn,
                                                  model_kwargs, device, progress, eta, resample, start_index, end_index, chain_noise,
                                                  blend_start, False))

    # ------------------------------------------------------------------ clips longer than num_frames (not in the reference)
    WINDOW_METHODS = ("ddim", "ddpm") + tuple(LINEAR_METHODS)

    def _window_loop(self, model, shape, noise, method, stride, clip_denoised, model_kwargs, eta, device, progress, step_noise,
                     num_frames, progressive):
        if method not in self.WINDOW_METHODS:
            raise LatteError(f"window_sample_loop: method must be one of {sorted(self.WINDOW_METHODS)}, got {method!r}")
        owner = self._engine_model(model)[0]
        F = num_frames or getattr(owner if owner is not None else getattr(model, "__self__", model), "num_frames", None)
        if F is None:
            raise LatteError("window_sample_loop: pass num_frames, the clip length of a model callable that (like the object it is "
                             "bound to) carries no num_frames")
        F = int(F)
        assert isinstance(shape, (tuple, list))
        if len(shape) != 5:
            raise LatteError("shape must be [N, L, C, H, W]")
        B, L, C, H, Wd = (int(v) for v in shape)
        stride = max(1, F // 2) if stride is None else int(stride)
        W = len(window_starts(L, F, stride))                       # refuses L < F and a stride outside 1 ... F
        if (H * Wd) % 4:
            raise LatteError("window_sample_loop: H * W must be a multiple of 4 (16-byte accesses of the window kernels)")
        linear = method in LINEAR_METHODS
        sch = plan = None
        if linear:
            sch = self.linear_scheduler(method)
            plan = np.ascontiguousarray(sch.engine_plan(), dtype=np.float64)
        _lib.require_gpu()
        model_kwargs = dict(model_kwargs or {})
        device = self._device(model, device, noise)
        img = noise if noise is not None else torch.randn(*shape, device=device)
        img = img.to(device=device, dtype=torch.float32).contiguous().clone()
        if tuple(img.shape) != (B, L, C, H, Wd):
            raise LatteError(f"window_sample_loop: noise must be {(B, L, C, H, Wd)}, got {tuple(img.shape)}")
        if linear:
            img = img * float(sch.init_noise_sigma)
        n = plan.shape[0] if linear else self.num_timesteps
        needs_noise = method == "ddpm" or (method == "ddim" and eta != 0.0)
        nz_all = None
        if step_noise is not None:
            if tuple(step_noise.shape) != (n,) + tuple(img.shape):
                raise LatteError(f"step_noise must be [{n}, ...latents]: one slab per denoiser evaluation of {method!r}")
            nz_all = step_noise.to(device=device, dtype=torch.float32).contiguous()
        ec = self._engine_chain(model, img, model_kwargs, windows=W)
        lib = load_library()
        if ec is not None and linear:
            # ---- whole chain inside the engine: one call, one trail
            check(lib.latte_engine_set_option(ec.eng, b"train_timesteps", self.original_num_steps))

            def call(first, last, trail, _):
                check(lib.latte_sample_plan_loop_windows(ec.eng, ec.uses_cfg, ec.cfg_scale, ptr(ec.x32), ptr(ec.y64), ec.B, n,
                                                         plan.ctypes.data, ptr(nz_all), trail, L, stride, stream_ptr()))
                return nz_all

            yield from self._engine_run(ec, 0, n - 1, n, progressive, call, x0_trail=False)
            return
        if ec is not None:
            # ---- whole chain inside the engine, in segments of consecutive steps as _loop segments its noise
            seg = max(1, min(n, self.SEGMENT_BYTES // max(ec.x32.numel() * 4, 1)))

            def call(i, lo, trail_s, trail_0):
                nz = None
                if needs_noise:   # row k of the segment is read at its k-th step: index i - k
                    nz = (nz_all[n - 1 - i:n - lo] if nz_all is not None
                          else torch.stack([torch.randn_like(ec.x32) for _ in range(i - lo + 1)])).contiguous()
                check(lib.latte_sample_loop_windows(ec.eng, self._h, _METHOD[method], float(eta), int(bool(clip_denoised)), ec.uses_cfg,
                                                    ec.cfg_scale, ptr(ec.x32), ptr(ec.y64), ec.B, i, lo, ptr(nz), trail_s, trail_0, L,
                                                    stride, stream_ptr()))
                return nz

            yield from self._engine_run(ec, n - 1, 0, seg, progressive, call)
            return
        # ---- generic model callable, step by step: gather, the model on the clips, latte_window_merge, the existing step
        kw = repeat_per_window(model_kwargs, B, W)

        def denoise(x, t):
            tt = torch.full((B * W,), t, device=x.device, dtype=torch.int64)
            out = model(window_gather(x, F, stride), tt, **kw)
            if isinstance(out, tuple):
                out = out[0]
            return window_merge(out.float().contiguous(), L, stride)

        if linear:
            for k, t in self._progress(list(enumerate(sch.timesteps.tolist())), progress):
                out = denoise(sch.scale_model_input(img, t).contiguous(), t)   # ORIGINAL timesteps, as _linear_loop
                if out.shape[2] not in (C, 2 * C):
                    raise AssertionError(f"model output has {out.shape[2]} channels for {C}-channel latents")
                img = sch.step(out[:, :, :C], t, img, return_dict=False, noise=None if nz_all is None else nz_all[k])[0]
                yield {"sample": img, "pred_xstart": None}
            return
        for k, i in enumerate(self._progress(list(range(n))[::-1], progress)):
            out = denoise(img, self.timestep_map[i])
            nz = None
            if needs_noise:
                nz = nz_all[k] if nz_all is not None else torch.randn_like(img)
            r = self._step(method, out, img, i, nz, eta, clip_denoised)
            yield r
            img = r["sample"]

    def window_sample_loop_progressive(self, model, shape, noise=None, method="ddim", stride=None, clip_denoised=True,
                                       model_kwargs=None, eta=0.0, device=None, progress=False, step_noise=None, num_frames=None):
        """``window_sample_loop`` yielding {"sample", "pred_xstart"} after every step (``pred_xstart`` is None for the linear
        methods, one item per denoiser evaluation)."""
        yield from self._window_loop(model, shape, noise, method, stride, clip_denoised, model_kwargs, eta, device, progress, step_noise,
                                     num_frames, True)

    def window_sample_loop(self, model, shape, noise=None, method="ddim", stride=None, clip_denoised=True, model_kwargs=None, eta=0.0,
                           device=None, progress=False, step_noise=None, num_frames=None):
        """A clip of ``shape`` = [N, L, C, H, W] with L >= the model's ``num_frames`` F, by temporal co-denoising on unchanged weights
        (Gen-L-Video / MultiDiffusion along time; not in the reference; F is read from the model or the object the callable is bound
        to, else ``num_frames`` gives it): at every denoiser evaluation the model runs on the
        W = ceil((L - F) / stride) + 1 overlapping F-frame windows of the long latent (``latte_amd.window_starts``; ``stride`` in
        1 ... F, default F // 2), the outputs are averaged with uniform weights where windows overlap, and ONE ordinary update of
        ``method`` -- "ddim" (``eta``), "ddpm", or a linear one ("euler", "euler_a", "heun", "dpmsolver++" on ``linear_scheduler``'s
        plan; ``clip_denoised`` and ``eta`` do not apply) -- is applied to the long latent.  L == F is the plain loop bit for bit.
        With ``model.forward`` / ``model.forward_with_cfg`` of a ``latte_amd.Latte`` and known kwargs the chain is ONE
        ``latte_sample_loop_windows`` call per segment / ONE ``latte_sample_plan_loop_windows`` call, every clip of the batch in
        one forward (the engine is sized to N * W clips); any other callable is called on the gathered clips with every
        ``model_kwargs`` tensor of leading dimension N repeated per window, then ``latte_window_merge`` and the existing step.
        ``step_noise`` [steps or evaluations, ...latents] gives the draws to either path in execution order; without it the
        DDPM / DDIM paths draw one ``torch.randn_like`` per step and "euler_a" draws as ``linear_sample_loop`` does.  No hooks and no
        known region.  Nothing is claimed about sample quality: the arithmetic is the stated scheme."""
        return self._last_sample(self._window_loop(model, shape, noise, method, stride, clip_denoised, model_kwargs, eta, device, progress,
                                                   step_noise, num_frames, False))

    # ------------------------------------------------------------------ DDIM inversion (gd:566-602)
    def _reverse_loop(self, model, x, clip_denoised, denoised_fn, cond_fn, model_kwargs, progress, start_index, end_index,
                      progressive):
        _lib.require_gpu()
        model_kwargs = dict(model_kwargs or {})
        start, end = self._index_range(start_index, end_index, ascending=True)
        img = x.to(dtype=torch.float32).contiguous().clone()
        if img.dim() != 5:
            raise LatteError("x must be [N, F, C, H, W]")
        ec = self._engine_chain(model, img, model_kwargs, denoised_fn is not None or cond_fn is not None)
        if ec is not None:
            # ---- whole range inside the engine (the dispatch rule of _loop); only progressive trails split it
            seg = end - start + 1
            if progressive:
                seg = max(1, min(seg, self.SEGMENT_BYTES // max(ec.x32.numel() * 4, 1)))
            lib = load_library()

            def call(i, hi, trail_s, trail_0):
                check(lib.latte_invert_loop(ec.eng, self._h, int(bool(clip_denoised)), ec.uses_cfg, ec.cfg_scale, ptr(ec.x32), ptr(ec.y64),
                                            ec.B, i, hi, trail_s, trail_0, stream_ptr()))

            yield from self._engine_run(ec, start, end, seg, progressive, call)
            return
        # ---- generic model callable, step by step
        for i in self._progress(list(range(start, end + 1)), progress):
            out = self._call_model(model, img, i, model_kwargs)
            r = self._step("ddim_reverse", out, img, i, None, 0.0, clip_denoised, denoised_fn, cond_fn, model_kwargs)
            yield r
            img = r["sample"]

    def ddim_reverse_sample_loop_progressive(self, model, x, clip_denoised=True, denoised_fn=None, cond_fn=None,
                                             model_kwargs=None, progress=False, start_index=0, end_index=None):
        """``ddim_reverse_sample_loop`` yielding every step's {"sample", "pred_xstart"} in execution order."""
        yield from self._reverse_loop(model, x, clip_denoised, denoised_fn, cond_fn, model_kwargs, progress, start_index,
                                      end_index, True)

    def ddim_reverse_sample_loop(self, model, x, clip_denoised=True, denoised_fn=None, cond_fn=None, model_kwargs=None,
                                 progress=False, start_index=0, end_index=None):
        """DDIM inversion of a clip ``x`` [N, F, C, H, W]: the reference has no such loop; this is the obvious
        ``for i in range(T)`` around its ``ddim_reverse_sample`` (gd:566-602), over the respaced indices ``start_index`` ...
        ``end_index`` ascending (default 0 ... T-1).  Index ``i`` evaluates the model at level ``i`` and carries ``x`` to level
        ``i + 1``; level T is pure noise, ONE level above where ``ddim_sample_loop`` starts (it takes its input as level T-1),
        so the way back from ``end_index = k - 1`` is ``ddim_sample_loop(..., noise=x_k, start_index=k)``.  With
        ``model.forward`` / ``model.forward_with_cfg`` of a ``latte_amd.Latte``, known kwargs and no hooks, the whole range is
        ONE ``latte_invert_loop`` call; any other callable is driven step by step.  Returns the inverted latent."""
        return self._last_sample(self._reverse_loop(model, x, clip_denoised, denoised_fn, cond_fn, model_kwargs, progress, start_index,
                                                    end_index, False))

    # ------------------------------------------------------------------ training path, forward evaluation
    def q_sample(self, x_start, t, noise=None):
        """``GaussianDiffusion.q_sample`` (gd:216-229) with one respaced timestep per sample, on the engine."""
        _lib.require_gpu()
        x0 = x_start.float().contiguous()
        if noise is None:
            noise = torch.randn_like(x0)
        if noise.shape != x0.shape:
            raise AssertionError("noise.shape == x_start.shape")                      # gd:225
        nz = noise.to(device=x0.device, dtype=torch.float32).contiguous()
        t64 = t.to(device=x0.device, dtype=torch.int64).contiguous()
        if t64.shape != (x0.shape[0],) or int(t64.min()) < 0 or int(t64.max()) >= self.num_timesteps:
            raise IndexError("t must hold one timestep index in [0, num_timesteps) per sample")
        out = torch.empty_like(x0)
        with torch.cuda.device(x0.device):
            check(load_library().latte_q_sample(self._h, ptr(x0), ptr(nz), ptr(t64), x0.shape[0], x0[0].numel(), ptr(out),
                                                stream_ptr()))
        return out

    def training_losses(self, model, x_start, t, model_kwargs=None, noise=None):
        """``SpacedDiffusion.training_losses`` (rs:95-98 -> gd:719-795) as called by train.py:224-226: the VALUES of the
        loss terms -- {"loss", "mse", "vb"} of shape [N] for the MSE loss types, {"loss"} for the KL ones -- computed by the
        engine from ``model(x_t, timestep_map[t], **model_kwargs)``.  Forward evaluation only: nothing here builds an
        autograd graph, the backward kernels are the next slice of SURVEY.md section 8(f) rank 3."""
        _lib.require_gpu()
        model_kwargs = model_kwargs or {}
        x0 = x_start.float().contiguous()
        if x0.dim() != 5:
            raise LatteError("x_start must be [N, F, C, H, W]")
        if noise is None:
            noise = torch.randn_like(x0)                                              # gd:732-733
        nz = noise.to(device=x0.device, dtype=torch.float32).contiguous()
        t64 = t.to(device=x0.device, dtype=torch.int64).contiguous()
        x_t = self.q_sample(x0, t64, nz)
        tmap = torch.tensor(self.timestep_map, device=x0.device, dtype=torch.int64)
        out = model(x_t, tmap[t64], **model_kwargs)                                  # rs:125-130: ORIGINAL timesteps
        if isinstance(out, tuple):
            out = out[0]
        B, F, C = x0.shape[:3]
        want = (B, F, C * 2 if self.learn_sigma else C, *x0.shape[3:])               # gd:762 / :784
        if tuple(out.shape) != want:
            raise AssertionError(f"model output shape {tuple(out.shape)} != {want}")
        mo = out.detach().float().contiguous()
        hw = int(np.prod(x0.shape[3:]))
        lib = load_library()
        nws = int(lib.latte_training_workspace_floats(B, x0[0].numel()))
        ws = torch.empty(nws, device=x0.device, dtype=torch.float32)
        mse, vb, loss = (torch.empty(B, device=x0.device, dtype=torch.float32) for _ in range(3))
        with torch.cuda.device(x0.device):
            check(lib.latte_training_losses(self._h, _LOSS[self.loss_type], ptr(x0), ptr(x_t), ptr(nz), ptr(mo), ptr(t64), B, F, C,
                                            hw, ptr(ws), nws, ptr(mse), ptr(vb), ptr(loss), stream_ptr()))
        if self.loss_type in ("kl", "rescaled_kl"):
            return {"loss": loss}
        terms = {"mse": mse, "loss": loss}
        if self.learn_sigma:
            terms["vb"] = vb
        return terms

    # ------------------------------------------------------------------ likelihood evaluation (gd:686-717, :797-866)
    def _prior_bpd(self, x_start):
        """``GaussianDiffusion._prior_bpd`` (gd:797-811): KL(q(x_T | x_0) || N(0, I)) in bits per dimension, [N]."""
        _lib.require_gpu()
        x0 = x_start.float().contiguous()
        out = torch.empty(x0.shape[0], device=x0.device, dtype=torch.float32)
        with torch.cuda.device(x0.device):
            check(load_library().latte_prior_bpd(self._h, ptr(x0), x0.shape[0], x0[0].numel(), ptr(out), stream_ptr()))
        return out

    def _bpd_terms(self, x0, x_t, noise, model_output, index, clip_denoised, tables=None, column=0, want_xstart=False):
        """One column of ``calc_bpd_loop`` on the engine (``latte_bpd_terms``): vb, xstart_mse, mse of respaced ``index`` into
        ``tables`` ([N, T] each) at ``column``, or into fresh [N] tensors."""
        B, F, C = x0.shape[:3]
        want = (B, F, C * 2 if self.learn_sigma else C, *x0.shape[3:])              # gd:290 / :338
        if tuple(model_output.shape) != want:
            raise AssertionError(f"model output shape {tuple(model_output.shape)} != {want}")
        mo = model_output.detach().to(device=x0.device, dtype=torch.float32).contiguous()
        if tables is None:
            tables = tuple(torch.empty(B, 1, device=x0.device, dtype=torch.float32) for _ in range(3))
            column = 0
        stride = tables[0].shape[1]
        hw = int(np.prod(x0.shape[3:]))
        lib = load_library()
        nws = int(lib.latte_bpd_workspace_floats(B, x0[0].numel()))
        ws = torch.empty(nws, device=x0.device, dtype=torch.float32)
        pred = torch.empty_like(x0) if want_xstart else None
        with torch.cuda.device(x0.device):
            check(lib.latte_bpd_terms(self._h, int(index), int(bool(clip_denoised)), ptr(x0), ptr(x_t), ptr(noise), ptr(mo), B, F, C, hw,
                                      ptr(ws), nws, ptr(tables[0][:, column:]), ptr(tables[1][:, column:]), ptr(tables[2][:, column:]),
                                      stride, ptr(pred), stream_ptr()))
        return tables, pred

    def _vb_terms_bpd(self, model, x_start, x_t, t, clip_denoised=True, model_kwargs=None):
        """``GaussianDiffusion._vb_terms_bpd`` (gd:686-717) for one timestep index shared by the batch, as ``calc_bpd_loop``
        calls it: {"output": KL (decoder NLL at t == 0) in bits [N], "pred_xstart"}.  The noise that made ``x_t`` is not an
        argument of the reference method; the eps-MSE column of the kernel is computed against zeros here and dropped."""
        _lib.require_gpu()
        index = self._uniform_index(t)
        x0 = x_start.float().contiguous()
        xt = x_t.to(device=x0.device, dtype=torch.float32).contiguous()
        out = self._call_model(model, xt, index, model_kwargs or {})
        tables, pred = self._bpd_terms(x0, xt, torch.zeros_like(x0), out, index, clip_denoised, want_xstart=True)
        return {"output": tables[0][:, 0], "pred_xstart": pred}

    def calc_bpd_loop(self, model, x_start, clip_denoised=True, model_kwargs=None, noise=None):
        """``GaussianDiffusion.calc_bpd_loop`` (gd:813-866): {"total_bpd", "prior_bpd" [N]; "vb", "xstart_mse", "mse" [N, T]},
        column 0 = t = T-1.  ``noise`` ([T, N, ...], row k for the k-th executed step) replaces the per-step draws of gd:837.
        With ``model`` the ``forward`` of a ``latte_amd.Latte`` the loop is ONE ``latte_bpd_loop`` call (its draws then come from
        the engine's Philox stream, option "seed"); any other callable is driven step by step with ``torch.randn_like`` draws."""
        _lib.require_gpu()
        model_kwargs = dict(model_kwargs or {})
        x0 = x_start.float().contiguous()
        if x0.dim() != 5:
            raise LatteError("x_start must be [N, F, C, H, W]")
        n = self.num_timesteps
        B = x0.shape[0]
        nz_all = None
        if noise is not None:
            if tuple(noise.shape) != (n,) + tuple(x0.shape):
                raise AssertionError("noise.shape == (num_timesteps,) + x_start.shape")
            nz_all = noise.to(device=x0.device, dtype=torch.float32).contiguous()
        tables = tuple(torch.empty(B, n, device=x0.device, dtype=torch.float32) for _ in range(3))
        owner, uses_cfg = self._engine_model(model)
        if owner is not None and not uses_cfg and owner.extras != 78 and set(model_kwargs) <= {"y", "use_fp16"}:
            # ---- whole loop inside the engine
            x0, _, y64 = owner._prep(x0, torch.zeros(B, dtype=torch.int64), model_kwargs.get("y"))
            eng = owner.engine(B)
            with torch.cuda.device(x0.device):
                check(load_library().latte_bpd_loop(eng, self._h, int(bool(clip_denoised)), ptr(x0), ptr(y64), B, n - 1, 0, ptr(nz_all),
                                                    ptr(tables[0]), ptr(tables[1]), ptr(tables[2]), stream_ptr()))
        else:
            # ---- generic model callable, step by step (gd:835-852)
            for k, i in enumerate(range(n - 1, -1, -1)):
                nz = nz_all[k] if nz_all is not None else torch.randn_like(x0)
                t = torch.full((B,), i, device=x0.device, dtype=torch.int64)
                x_t = self.q_sample(x0, t, nz)
                out = self._call_model(model, x_t, i, model_kwargs)
                self._bpd_terms(x0, x_t, nz, out, i, clip_denoised, tables, k)
        vb, xstart_mse, mse = tables
        prior_bpd = self._prior_bpd(x0)
        total_bpd = vb.sum(dim=1) + prior_bpd                                       # gd:859
        return {"total_bpd": total_bpd, "prior_bpd": prior_bpd, "vb": vb, "xstart_mse": xstart_mse, "mse": mse}


def create_diffusion(timestep_respacing, noise_schedule="linear", use_kl=False, sigma_small=False,
                     predict_xstart=False, learn_sigma=True, rescale_learned_sigmas=False, diffusion_steps=1000):
    """``diffusion.create_diffusion`` (diffusion/__init__.py:10-47).  ``use_kl`` / ``rescale_learned_sigmas`` select the
    training loss (LossType RESCALED_KL / RESCALED_MSE / MSE, :22-27) and do not touch sampling."""
    if timestep_respacing is None or timestep_respacing == "":
        timestep_respacing = [diffusion_steps]
    loss_type = "rescaled_kl" if use_kl else ("rescaled_mse" if rescale_learned_sigmas else "mse")
    return SpacedDiffusion(timestep_respacing, noise_schedule=noise_schedule, diffusion_steps=diffusion_steps,
                           predict_xstart=predict_xstart, learn_sigma=learn_sigma, sigma_small=sigma_small, loss_type=loss_type)
