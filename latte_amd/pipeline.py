"""``LattePipeline`` of ``sample/pipeline_latte.py`` (:100-115 constructor, :516-798 ``__call__``) around the MI355X
denoiser: the sampling loop of Latte-1 text-to-video.

What runs where: the transformer call of every step (``latte_amd.LatteT2V``, the hot path) and the VAE decode
(``latte_amd.AutoencoderKL``) run on the HIP engine.  The text encoder / tokenizer are whatever the caller passes (a
``transformers`` T5 in the reference) or are bypassed with ``prompt_embeds`` / ``negative_prompt_embeds``; the scheduler is
any object with the diffusers interface (``latte_amd.schedulers.DDIMScheduler`` is a self-contained stand-in).  With that
scheduler at eta = 0 the whole guided loop (:700-760) runs inside the engine (``latte_t2v_guided_ddim_loop``: text context
computed once, guidance combine + learned-sigma drop + DDIM update fused into one kernel per step), and so does the chain of a
scheduler that exposes ``engine_plan()`` (Euler, Euler-ancestral, Heun, DPM-Solver++ of ``latte_amd.schedulers``:
``latte_t2v_guided_linear_loop``); with any other scheduler object the guidance combine, the learned-sigma drop and the scheduler update are the reference's own few
elementwise lines (:747-758) on device tensors around the engine denoiser.  ``enable_vae_temporal_decoder=True`` decodes through
``latte_amd.AutoencoderKLTemporalDecoder`` in chunks of 14 frames (:779-798), else per frame (:765-777).
"""
import inspect

import torch

from ._lib import LatteError


class VideoPipelineOutput:
    def __init__(self, video):
        self.video = video


class LattePipeline:
    def __init__(self, tokenizer=None, text_encoder=None, vae=None, transformer=None, scheduler=None):
        if transformer is None or scheduler is None:
            raise LatteError("LattePipeline needs at least a transformer (latte_amd.LatteT2V) and a scheduler")
        self.tokenizer, self.text_encoder, self.vae, self.transformer, self.scheduler = tokenizer, text_encoder, vae, transformer, scheduler
        self.vae_scale_factor = 2 ** (len(vae.config.block_out_channels) - 1) if vae is not None else 8   # pipeline_latte.py:114
        self._device = getattr(transformer, "_device", torch.device("cuda"))

    def to(self, device):
        self._device = torch.device(device)
        for m in (self.transformer, self.vae, self.text_encoder):
            if m is not None and hasattr(m, "to"):
                m.to(device)
        return self

    # ------------------------------------------------------------------ pipeline_latte.py:117-126
    @staticmethod
    def mask_text_embeddings(emb, mask):
        if emb.shape[0] == 1:
            keep_index = int(mask.sum().item())
            return emb[:, :, :keep_index, :], keep_index
        return emb * mask[:, None, :, None], emb.shape[2]

    # ------------------------------------------------------------------ pipeline_latte.py:359-379
    @staticmethod
    def _text_preprocessing(text, clean_caption=False):
        """What the reference does to every prompt AND negative prompt before the tokenizer (T5 is case sensitive, so
        skipping it changes the token ids): ``text.lower().strip()``, or -- with ``clean_caption`` and both ``bs4`` and
        ``ftfy`` importable -- diffusers' DeepFloyd-IF ``_clean_caption`` twice.  That cleaner (a battery of url / html /
        CJK / punctuation regexes, pipeline_latte.py:384-496) is not restated here: ``clean_caption=True`` warns and takes
        the ``lower().strip()`` path, which is also what the reference itself does whenever one of the two packages is
        missing (:360-368) -- the case in this image."""
        if clean_caption:
            import warnings
            warnings.warn("latte_amd.LattePipeline: clean_caption=True is not available (diffusers' _clean_caption is not "
                          "restated); prompts are lower-cased and stripped, as the reference does without bs4 / ftfy")
        if not isinstance(text, (tuple, list)):
            text = [text]
        return [str(t).lower().strip() for t in text]

    # ------------------------------------------------------------------ pipeline_latte.py:127-270
    def encode_prompt(self, prompt, do_classifier_free_guidance=True, negative_prompt="", num_images_per_prompt=1, device=None,
                      prompt_embeds=None, negative_prompt_embeds=None, clean_caption=False, mask_feature=True):
        embeds_initially_provided = prompt_embeds is not None and negative_prompt_embeds is not None
        device = device or self._device
        if prompt is not None and isinstance(prompt, str):
            prompt = [prompt]
        batch_size = len(prompt) if prompt is not None else prompt_embeds.shape[0]
        max_length = 120
        if prompt_embeds is None:
            if self.tokenizer is None or self.text_encoder is None:
                raise LatteError("pass prompt_embeds / negative_prompt_embeds, or construct the pipeline with a tokenizer and a "
                                 "text encoder (T5 in the reference)")
            prompt = self._text_preprocessing(prompt, clean_caption=clean_caption)                 # :182
            ti = self.tokenizer(prompt, padding="max_length", max_length=max_length, truncation=True, return_attention_mask=True,
                                add_special_tokens=True, return_tensors="pt")
            attention_mask = ti.attention_mask.to(device)
            prompt_embeds_attention_mask = attention_mask
            prompt_embeds = self.text_encoder(ti.input_ids.to(device), attention_mask=attention_mask)[0]
        else:
            prompt_embeds_attention_mask = torch.ones_like(prompt_embeds)
        prompt_embeds = prompt_embeds.to(device=device, dtype=torch.float32)
        bs_embed, seq_len, _ = prompt_embeds.shape
        prompt_embeds = prompt_embeds.repeat(1, num_images_per_prompt, 1).view(bs_embed * num_images_per_prompt, seq_len, -1)
        prompt_embeds_attention_mask = prompt_embeds_attention_mask.view(bs_embed, -1).repeat(num_images_per_prompt, 1)
        if do_classifier_free_guidance and negative_prompt_embeds is None:
            uncond_tokens = self._text_preprocessing([negative_prompt] * batch_size, clean_caption=clean_caption)   # :230-231
            ui = self.tokenizer(uncond_tokens, padding="max_length", max_length=prompt_embeds.shape[1],
                                truncation=True, return_attention_mask=True, add_special_tokens=True, return_tensors="pt")
            negative_prompt_embeds = self.text_encoder(ui.input_ids.to(device), attention_mask=ui.attention_mask.to(device))[0]
        if do_classifier_free_guidance:
            seq_len = negative_prompt_embeds.shape[1]
            negative_prompt_embeds = negative_prompt_embeds.to(device=device, dtype=torch.float32)
            negative_prompt_embeds = negative_prompt_embeds.repeat(1, num_images_per_prompt, 1).view(
                batch_size * num_images_per_prompt, seq_len, -1)
        else:
            negative_prompt_embeds = None
        if mask_feature and not embeds_initially_provided:
            masked, keep = self.mask_text_embeddings(prompt_embeds.unsqueeze(1), prompt_embeds_attention_mask)
            neg = negative_prompt_embeds[:, :keep, :] if negative_prompt_embeds is not None else None
            return masked.squeeze(1), neg
        return prompt_embeds, negative_prompt_embeds

    def _ddim_tables(self, steps):
        """(timesteps, alpha_t, alpha_prev) of the DDIM scheduler's steps, as the engine's guided DDIM loops take them."""
        sch = self.scheduler
        ts = [int(t) for t in steps]
        ratio = sch.num_train_timesteps // sch.num_inference_steps
        a_t = [float(sch.alphas_cumprod[t]) for t in ts]
        a_p = [float(sch.alphas_cumprod[t - ratio]) if t - ratio >= 0 else float(sch.final_alpha_cumprod) for t in ts]
        return ts, a_t, a_p

    def _fused_loop(self, steps, do_cfg, eta, callback, latent_channels):
        """(timesteps, alpha_t, alpha_prev) when the loop can run inside the engine (latte_t2v_guided_ddim_loop): guidance on,
        the self-contained DDIM scheduler at eta = 0 without clipping, the engine transformer, no per-step callback.  Any
        other scheduler object / configuration takes the step-by-step loop below."""
        from .schedulers import DDIMScheduler
        from .t2v import LatteT2V
        sch, tr = self.scheduler, self.transformer
        if not (do_cfg and callback is None and eta == 0.0 and type(sch) is DDIMScheduler and not sch.clip_sample
                and isinstance(tr, LatteT2V) and tr.config.out_channels in (latent_channels, 2 * latent_channels)
                and getattr(self, "allow_fused_loop", True)):
            return None
        return self._ddim_tables(steps)

    def _known_loop(self, latents, known, mask, steps, prompt_embeds, do_cfg, guidance_scale, eta, generator, callback, callback_steps,
                    enable_temporal_attentions):
        """The denoising loop with the known part of the latents replaced: ONE
        ``latte_t2v_guided_ddim_loop_known`` call when guidance is on, there is no callback and ``allow_fused_loop`` is set; else the
        step-by-step loop with one ``latte_known_blend`` launch before the first step and after every step."""
        import numpy as np
        from .known import known_blend
        from .schedulers import DDIMScheduler, draw_noise
        from .t2v import LatteT2V
        sch, tr = self.scheduler, self.transformer
        if type(sch) is not DDIMScheduler or eta != 0.0 or sch.clip_sample:
            raise LatteError("known_latents: known-region sampling runs on latte_amd.DDIMScheduler at eta = 0 without clipping only -- the "
                             "samples of the other schedulers live at other noise levels and Heun has intermediate states")
        cfg = tr.config
        device = latents.device
        b, C, F, H, W = latents.shape
        known = known.to(device=device, dtype=torch.float32).contiguous()
        mask = mask.to(device=device, dtype=torch.float32).contiguous()
        if known.shape != latents.shape or tuple(mask.shape) != (b, F, H, W):
            raise LatteError(f"known_latents must be {tuple(latents.shape)} and known_mask {(b, F, H, W)}, got {tuple(known.shape)} and "
                             f"{tuple(mask.shape)}")
        if (H * W) % 4:
            raise LatteError("known_latents: h * w must be a multiple of 4 (16-byte accesses of the blend kernel)")
        ts, a_t, a_p = self._ddim_tables(steps)
        # slab 0: the blend before step 0; slab k + 1: the blend after step k (the last step takes none)
        noise = torch.stack([draw_noise(latents.shape, generator, device, latents.dtype) for _ in ts])
        if (do_cfg and callback is None and isinstance(tr, LatteT2V) and cfg.out_channels in (C, 2 * C)
                and getattr(self, "allow_fused_loop", True)):
            tr.set_text(prompt_embeds)
            return tr.guided_ddim_loop_known(latents, ts, a_t, a_p, guidance_scale, known, mask, noise, enable_temporal_attentions)

        def blend(x, abar, z):   # the engine's coefficients: fp64 square roots narrowed to fp32
            a, bb = (1.0, 0.0) if z is None else (float(np.float32(np.sqrt(abar))), float(np.float32(np.sqrt(1.0 - abar))))
            return known_blend(x.to(dtype=torch.float32).contiguous(), known, mask, a, bb, z, frames_inner=True)

        added_cond_kwargs = {"resolution": None, "aspect_ratio": None}
        latents = blend(latents.clone(), a_t[0], noise[0])
        for i, t in enumerate(steps):
            x_in = sch.scale_model_input(torch.cat([latents] * 2) if do_cfg else latents, t)
            current = t if torch.is_tensor(t) else torch.tensor([t], dtype=torch.int64, device=device)
            current = current.reshape(-1)[:1].to(device).expand(x_in.shape[0])
            noise_pred = tr(x_in, encoder_hidden_states=prompt_embeds, timestep=current, added_cond_kwargs=added_cond_kwargs,
                            enable_temporal_attentions=enable_temporal_attentions, return_dict=False)[0]
            if do_cfg:
                uncond, text = noise_pred.chunk(2)
                noise_pred = uncond + guidance_scale * (text - uncond)
            if cfg.out_channels // 2 == C:
                noise_pred = noise_pred.chunk(2, dim=1)[0]
            latents = sch.step(noise_pred, t, latents, eta=0.0, return_dict=False)[0]
            latents = blend(latents, a_p[i], noise[i + 1] if i + 1 < len(ts) else None)
            if callback is not None and i % callback_steps == 0:
                callback(i, t, latents)
        return latents

    def _fused_plan(self, do_cfg, callback, latent_channels, scheduler=None):
        """The scheduler's ``engine_plan()`` table when the chain can run inside the engine as latte_t2v_guided_linear_loop: guidance
        on, no per-step callback, the engine transformer, a scheduler that describes its update as such a table (Euler,
        Euler-ancestral, Heun, DPM-Solver++ of latte_amd.schedulers).  Else None: the step-by-step loop."""
        from .t2v import LatteT2V
        sch, tr = scheduler or self.scheduler, self.transformer
        if not (do_cfg and callback is None and getattr(self, "allow_fused_loop", True) and isinstance(tr, LatteT2V)
                and tr.config.out_channels in (latent_channels, 2 * latent_channels) and hasattr(sch, "engine_plan")):
            return None
        return sch.engine_plan()

    def prepare_latents(self, batch_size, num_channels_latents, video_length, height, width, device, generator, latents=None):
        shape = (batch_size, num_channels_latents, video_length, height // self.vae_scale_factor, width // self.vae_scale_factor)
        if latents is None:
            gdev = generator.device if generator is not None else device
            latents = torch.randn(shape, generator=generator, device=gdev, dtype=torch.float32).to(device)
        else:
            latents = latents.to(device=device, dtype=torch.float32)
        return latents * self.scheduler.init_noise_sigma                                       # pipeline_latte.py:513

    # ------------------------------------------------------------------ pipeline_latte.py:773-785
    def decode_latents(self, latents):
        if self.vae is None:
            raise LatteError("decode_latents needs a VAE (latte_amd.AutoencoderKL)")
        b, c, f, h, w = latents.shape
        z = (1.0 / self.vae.config.scaling_factor) * latents.permute(0, 2, 1, 3, 4).reshape(b * f, c, h, w)
        video = self.vae.decode(z.contiguous()).sample                                         # all frames in one engine call
        video = video.reshape(b, f, *video.shape[1:]).permute(0, 1, 3, 4, 2)                    # '(b f) c h w -> b f h w c'
        return ((video / 2.0 + 0.5).clamp(0, 1) * 255).to(dtype=torch.uint8).cpu().contiguous()

    def decode_latents_with_temporal_decoder(self, latents):
        """pipeline_latte.py:779-798: chunks of 14 frames through ``vae.decode(chunk, num_frames=len(chunk))``."""
        if not getattr(self.vae, "_TEMPORAL", False):
            raise LatteError("decode_latents_with_temporal_decoder needs a latte_amd.AutoencoderKLTemporalDecoder")
        b, c, f, h, w = latents.shape
        z = (1.0 / self.vae.config.scaling_factor) * latents.permute(0, 2, 1, 3, 4).reshape(b * f, c, h, w)
        video = []
        decode_chunk_size = 14
        for i in range(0, z.shape[0], decode_chunk_size):
            chunk = z[i:i + decode_chunk_size].contiguous()
            video.append(self.vae.decode(chunk, num_frames=chunk.shape[0]).sample)
        video = torch.cat(video)
        video = video.reshape(b, f, *video.shape[1:]).permute(0, 1, 3, 4, 2)
        return ((video / 2.0 + 0.5).clamp(0, 1) * 255).to(dtype=torch.uint8).cpu().contiguous()

    # ------------------------------------------------------------------ DDIM inversion (no counterpart in pipeline_latte.py)
    @torch.no_grad()
    def invert(self, prompt=None, latents=None, num_inference_steps=50, guidance_scale=1.0, negative_prompt="", prompt_embeds=None,
               negative_prompt_embeds=None, enable_temporal_attentions=True, clean_caption=True, mask_feature=True):
        """DDIM inversion of clean ``latents`` [B, 4, F, h, w] under a prompt: ``DDIMInverseScheduler`` (``self.inverse_scheduler``,
        default ``DDIMInverseScheduler()``) for ``num_inference_steps`` evaluations -> latents at level abar[u_{n-1}], where
        ``__call__(latents=..., num_inference_steps=n)`` with the DDIM scheduler starts.  Guidance above 1 runs the whole chain
        inside the engine (``latte_t2v_guided_linear_loop``); otherwise ``LatteT2V.forward`` is stepped from Python without a
        guidance pair.  The prompt is encoded and the text context installed as in ``__call__``."""
        from .schedulers import DDIMInverseScheduler
        if latents is None:
            raise ValueError("invert needs the clean `latents` [B, 4, F, h, w] of the clip")
        if prompt is None and prompt_embeds is None:
            raise ValueError("Provide either `prompt` or `prompt_embeds`.")
        cfg = self.transformer.config
        device = self._device
        latents = latents.to(device=device, dtype=torch.float32)
        if latents.dim() != 5 or latents.shape[1] != cfg.in_channels:
            raise ValueError(f"latents must be [B, {cfg.in_channels}, F, h, w], got {tuple(latents.shape)}")
        prompts = 1 if isinstance(prompt, str) else len(prompt) if prompt is not None else prompt_embeds.shape[0]
        if prompts != latents.shape[0]:
            raise ValueError(f"one prompt per clip: {prompts} prompts for {latents.shape[0]} clips")
        do_cfg = guidance_scale > 1.0
        prompt_embeds, negative_prompt_embeds = self.encode_prompt(
            prompt, do_cfg, negative_prompt=negative_prompt, device=device, prompt_embeds=prompt_embeds,
            negative_prompt_embeds=negative_prompt_embeds, clean_caption=clean_caption, mask_feature=mask_feature)
        if do_cfg:
            prompt_embeds = torch.cat([negative_prompt_embeds, prompt_embeds], dim=0)
        sch = getattr(self, "inverse_scheduler", None) or DDIMInverseScheduler()
        sch.set_timesteps(num_inference_steps, device=device)
        plan = self._fused_plan(do_cfg, None, cfg.in_channels, scheduler=sch)
        if plan is not None:
            self.transformer.set_text(prompt_embeds)
            return self.transformer.guided_linear_loop(latents, plan, None, guidance_scale, enable_temporal_attentions)
        added_cond_kwargs = {"resolution": None, "aspect_ratio": None}
        for t in sch.timesteps:
            x_in = sch.scale_model_input(torch.cat([latents] * 2) if do_cfg else latents, t)
            current = t.reshape(-1)[:1].to(device).expand(x_in.shape[0])
            noise_pred = self.transformer(x_in, encoder_hidden_states=prompt_embeds, timestep=current, added_cond_kwargs=added_cond_kwargs,
                                          enable_temporal_attentions=enable_temporal_attentions, return_dict=False)[0]
            if do_cfg:
                uncond, text = noise_pred.chunk(2)
                noise_pred = uncond + guidance_scale * (text - uncond)
            if cfg.out_channels // 2 == cfg.in_channels:
                noise_pred = noise_pred.chunk(2, dim=1)[0]
            latents = sch.step(noise_pred, t, latents, return_dict=False)[0]
        return latents

    # ------------------------------------------------------------------ pipeline_latte.py:516-771
    @torch.no_grad()
    def __call__(self, prompt=None, negative_prompt="", num_inference_steps=20, timesteps=None, guidance_scale=4.5,
                 num_images_per_prompt=1, video_length=None, height=None, width=None, eta=0.0, generator=None, latents=None,
                 prompt_embeds=None, negative_prompt_embeds=None, output_type="pil", return_dict=True, callback=None,
                 callback_steps=1, clean_caption=True, mask_feature=True, enable_temporal_attentions=True,
                 enable_vae_temporal_decoder=False, known_latents=None, known_mask=None, window_stride=None):
        """``window_stride`` (not in the reference; None = off): ``video_length`` may exceed the transformer's by temporal co-denoising --
        at every step the transformer runs on the overlapping windows of the long latents (``latte_amd.window_starts``), the
        prompt embeddings repeated per window, and the window outputs are averaged before the scheduler's one update (DESIGN.md
        section 4.10e).  The chain runs inside the engine under the rule of the plain call; decode covers every frame.
        ``known_latents`` [B, 4, F, h, w] with ``known_mask`` [B, F, h, w] (``latte_amd.known_mask``; 1 = known) hold part of the clip
        fixed and generate the rest (not in the reference): before the first step and after every step the known part of the latents
        is overwritten with ``known_latents`` diffused to the level the latents are at, the clean ones after the last step.  DDIM
        scheduler of latte_amd at eta = 0 only; the noise comes from ``generator``, one latent-shaped draw per step, in slab order."""
        if (known_latents is None) != (known_mask is None):
            raise LatteError("known_latents and known_mask come together")
        if window_stride is not None and known_latents is not None:
            raise LatteError("window_stride: no known-region sampling on a windowed clip")
        if enable_vae_temporal_decoder and not getattr(self.vae, "_TEMPORAL", False):
            raise LatteError("enable_vae_temporal_decoder=True needs a latte_amd.AutoencoderKLTemporalDecoder as the pipeline's vae "
                             "(sample_t2x.py:31-32 loads it from subfolder 'vae_temporal_decoder')")
        cfg = self.transformer.config
        height = height or cfg.sample_size * self.vae_scale_factor
        width = width or cfg.sample_size * self.vae_scale_factor
        video_length = video_length or cfg.video_length
        if prompt is None and prompt_embeds is None:
            raise ValueError("Provide either `prompt` or `prompt_embeds`.")
        if prompt is not None and isinstance(prompt, str):
            batch_size = 1
        elif prompt is not None:
            batch_size = len(prompt)
        else:
            batch_size = prompt_embeds.shape[0]
        device = self._device
        do_cfg = guidance_scale > 1.0
        prompt_embeds, negative_prompt_embeds = self.encode_prompt(
            prompt, do_cfg, negative_prompt=negative_prompt, num_images_per_prompt=num_images_per_prompt, device=device,
            prompt_embeds=prompt_embeds, negative_prompt_embeds=negative_prompt_embeds, clean_caption=clean_caption,
            mask_feature=mask_feature)
        if do_cfg:
            prompt_embeds = torch.cat([negative_prompt_embeds, prompt_embeds], dim=0)             # :647
        self.scheduler.set_timesteps(num_inference_steps, device=device)
        steps = self.scheduler.timesteps
        latent_channels = cfg.in_channels
        latents = self.prepare_latents(batch_size * num_images_per_prompt, latent_channels, video_length, height, width, device,
                                       generator, latents)
        extra = {}
        params = set(inspect.signature(self.scheduler.step).parameters.keys())
        if "eta" in params:
            extra["eta"] = eta
        if "generator" in params:
            extra["generator"] = generator
        added_cond_kwargs = {"resolution": None, "aspect_ratio": None}
        tr = self.transformer
        if window_stride is not None:
            from .windows import window_gather, window_merge, window_starts
            if latents.dim() != 5 or (latents.shape[3] * latents.shape[4]) % 4:
                raise LatteError("window_stride: latents must be [b, C, L, h, w] with h * w a multiple of 4")
            window_stride = int(window_stride)
            windows = len(window_starts(latents.shape[2], cfg.video_length, window_stride))   # refuses a bad length / stride
            prompt_embeds = prompt_embeds.repeat_interleave(windows, dim=0)                   # row g W + w = row g: [negative | prompt] kept
        if known_latents is not None:
            latents = self._known_loop(latents, known_latents, known_mask, steps, prompt_embeds, do_cfg, guidance_scale, eta, generator,
                                       callback, callback_steps, enable_temporal_attentions)
            steps = []
        fused = self._fused_loop(steps, do_cfg, eta, callback, latent_channels) if known_latents is None else None
        if fused is not None:
            # the whole guided DDIM chain inside the engine: no torch op between the first and the last step
            tr.set_text(prompt_embeds)
            if window_stride is None:
                latents = tr.guided_ddim_loop(latents, fused[0], fused[1], fused[2], guidance_scale, enable_temporal_attentions)
            else:
                latents = tr.guided_ddim_loop_windows(latents, fused[0], fused[1], fused[2], guidance_scale, window_stride,
                                                      enable_temporal_attentions)
            steps = []
        plan = self._fused_plan(do_cfg, callback, latent_channels) if fused is None and known_latents is None else None
        if plan is not None:
            # the same chain for every sampler with a linear update: one table, one engine call.  A stochastic sampler's noise is
            # drawn up front by the calls its step() would make, in order, so both loops consume the generator alike
            noise = None
            from .schedulers import P_CN, draw_noise
            if (plan[:, P_CN] != 0.0).any():
                noise = torch.stack([draw_noise(latents.shape, generator, device, latents.dtype) for _ in range(plan.shape[0])])
            tr.set_text(prompt_embeds)
            if window_stride is None:
                latents = tr.guided_linear_loop(latents, plan, noise, guidance_scale, enable_temporal_attentions)
            else:
                latents = tr.guided_linear_loop_windows(latents, plan, noise, guidance_scale, window_stride, enable_temporal_attentions)
            steps = []
        for i, t in enumerate(steps):
            latent_model_input = torch.cat([latents] * 2) if do_cfg else latents
            latent_model_input = self.scheduler.scale_model_input(latent_model_input, t)
            current = t if torch.is_tensor(t) else torch.tensor([t], dtype=torch.int64, device=device)
            if window_stride is not None:   # the clips of every row of the (doubled) batch
                latent_model_input = window_gather(latent_model_input.to(dtype=torch.float32).contiguous(), cfg.video_length,
                                                   window_stride, frames_inner=True)
            current = current.reshape(-1)[:1].to(device).expand(latent_model_input.shape[0])
            noise_pred = self.transformer(latent_model_input, encoder_hidden_states=prompt_embeds, timestep=current,
                                          added_cond_kwargs=added_cond_kwargs,
                                          enable_temporal_attentions=enable_temporal_attentions, return_dict=False)[0]
            if window_stride is not None:
                noise_pred = window_merge(noise_pred.to(dtype=torch.float32).contiguous(), latents.shape[2], window_stride,
                                          frames_inner=True)
            if do_cfg:
                uncond, text = noise_pred.chunk(2)
                noise_pred = uncond + guidance_scale * (text - uncond)                           # :748-749
            if cfg.out_channels // 2 == latent_channels:
                noise_pred = noise_pred.chunk(2, dim=1)[0]                                        # learned sigma dropped, :752-753
            latents = self.scheduler.step(noise_pred, t, latents, **extra, return_dict=False)[0]
            if callback is not None and i % callback_steps == 0:
                callback(i // getattr(self.scheduler, "order", 1), t, latents)
        if output_type == "latents":
            video = latents
        elif enable_vae_temporal_decoder:                                                 # pipeline_latte.py:737-740
            video = self.decode_latents_with_temporal_decoder(latents)
        else:
            video = self.decode_latents(latents)
        return VideoPipelineOutput(video=video) if return_dict else (video,)
