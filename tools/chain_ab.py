"""A/B of two builds of the library, or of two trees with their front ends, on the engine's fused loops: every loop on fixed seeds,
sha256 of every returned tensor.

  python tools/chain_ab.py --out profiles/chain_refactor_head.json                                   # the tree's library
  LATTE_AMD_LIB=<other build>.so python tools/chain_ab.py --out profiles/chain_refactor_parent.json  # another build
  python tools/chain_ab.py --tree <built checkout of another commit> --out profiles/known_refactor_parent.json   # library AND front end
  python tools/chain_ab.py --compare profiles/chain_refactor_parent.json profiles/chain_refactor_head.json

Builds nothing: it loads LATTE_AMD_LIB or latte_amd/lib/liblatte_amd.so of the tree ``latte_amd`` and ``tests/_util`` are imported from
(--tree, default this one).  Models: the tiny_classcond and tiny_uncond golden fixtures
(f16 operands, max_batch 4) and the tiny text-to-video pipeline of tests/test_t2v_schedulers.py.  Cases:
  sample loop   DDPM, DDIM eta 0 and eta 0.5 with both trails, noise drawn by the engine (option "seed"); on the class-conditional model
                guided at batch 4 over 70 steps (bu = 4: the conditioning chunk holds 64), once whole and once as two segments
  invert loop   the same range, whole and split, both trails
  bpd loop      given noise and drawn noise, both models
  plan loop     Euler, Euler-ancestral (drawn noise), Heun, DPM-Solver++ on create_diffusion("6"), guided and plain, with the trail; Heun
                on create_diffusion("40") (79 rows, guided batch 4).  Euler / Heun scale the model input.
  T2V           latte_t2v_guided_linear_loop for the four methods and the guided DDIM loop, through LattePipeline; the known-region DDIM
                loop through LattePipeline(known_latents=, known_mask=)
  known loop    latte_sample_loop_known for DDPM, DDIM eta 0 and eta 0.5 at resample 1 and 2, both trails: guided batch 4 over 70 steps
                whole and as two calls (blend_start on the first only), plain batch 3, unconditional batch 2; each with noise drawn by the
                engine and with given slabs
  forward       (--only forward runs it alone) one denoiser forward per case on models of XL width and depth 2, where the block's shape
                rules reach every kernel: Latte at B = 1, 2, 8 under the engine options that select a block-level path (gated_split_k,
                stream_policy, gated_rmw_shape, fc2_temp_embed, gemm_variant_fc2, fuse_qkv_attn), forward_with_cfg under guided_split
                0 / 3 / 12 / 20 with "guided_split_active" read back, bf16, the three tiny fixtures; LatteT2V (one layer, 20 text tokens,
                partly masked) at 256-token x 16-frame, 1024-token x 16-frame and single-frame geometries, temporal blocks on and off.
                Values cannot show WHICH kernel ran where two give the same bits: run it under
                ``rocprofv3 --kernel-trace --stats`` and compare the name -> calls tables (profiles/block_body_kernel_stats_*.csv)
  front end     p_sample_loop_progressive, ddim_reverse_sample_loop_progressive and known_sample_loop_progressive of SpacedDiffusion
                on torch.manual_seed draws with SEGMENT_BYTES cut to three indices per engine call
After every class-engine case the option "seed" is read back and one further engine-drawn DDPM step is hashed, so the Philox offset
must have advanced identically.  Two runs agree when every hash agrees."""
import argparse
import hashlib
import json
import os
import sys

import numpy as np
import torch

_pre = argparse.ArgumentParser(add_help=False)
_pre.add_argument("--tree")
ROOT = os.path.abspath(_pre.parse_known_args()[0].tree or os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import latte_amd  # noqa: E402
from latte_amd._lib import check, load_library, ptr, stream_ptr  # noqa: E402

DDPM, DDIM = 0, 1
LINEAR = ["euler", "euler_a", "heun", "dpmsolver++"]
CFG = 4.0


def sha(t):
    """sha256 of the tensor's bytes; a tensor with a non-finite element is marked, so that a chain that left the fp32 range shows"""
    torch.cuda.synchronize()
    t = t.detach().cpu().contiguous()
    return ("" if bool(torch.isfinite(t).all()) else "nonfinite:") + hashlib.sha256(t.numpy().tobytes()).hexdigest()


class ClassEngine:
    def __init__(self, name):
        from _util import engine_model, load_golden_model
        kw, sd, _ = load_golden_model(name)
        self.name, self.m = name, engine_model(kw, sd, "f16", max_batch=4)
        self.shape = (kw["num_frames"], 4, kw["input_size"], kw["input_size"])
        self.classes = kw["num_classes"] if kw["extras"] == 2 else None
        self.lib = load_library()

    def inputs(self, B, guided, seed):
        g = torch.Generator("cpu").manual_seed(seed)
        half = B // 2 if guided else B
        x = torch.randn((half,) + self.shape, generator=g)
        y = None
        if self.classes is not None:
            y = torch.randint(0, self.classes, (half,), generator=g)
            if guided:
                y = torch.cat([y, torch.full_like(y, self.classes)])
            y = y.cuda()
        if guided:
            x = torch.cat([x, x])
        return x.cuda().contiguous(), y

    def tail(self, rec, B, guided, d, y):
        """option "seed" + one further engine-drawn DDPM step: the continuation of the noise stream"""
        rec["seed_after"] = self.m.get_engine_option("seed", batch=B, guided=guided)
        x = torch.full((B,) + self.shape, 0.25, device="cuda")
        check(self.lib.latte_sample_loop_ex(self.m.engine(B, guided), d._h, DDPM, 0.0, 1, int(guided), CFG, ptr(x), ptr(y), B, 1, 1, None,
                                            None, None, stream_ptr()))
        rec["next_drawn_step"] = sha(x)

    def sample(self, d, method, eta, B, guided, segments, seed, invert=False):
        x, y = self.inputs(B, guided, seed)
        self.m.set_engine_option("seed", seed, batch=B, guided=guided)
        eng, rec = self.m.engine(B, guided), {}
        n = sum(hi - lo + 1 for lo, hi in segments)
        trail_s = torch.empty((n,) + tuple(x.shape), device="cuda")
        trail_0 = torch.empty_like(trail_s)
        k = 0
        for lo, hi in segments:          # descending chains run hi ... lo, the inversion lo ... hi
            if invert:
                check(self.lib.latte_invert_loop(eng, d._h, 1, int(guided), CFG, ptr(x), ptr(y), B, lo, hi, ptr(trail_s[k:]), ptr(trail_0[k:]),
                                                 stream_ptr()))
            else:
                check(self.lib.latte_sample_loop_ex(eng, d._h, method, eta, 1, int(guided), CFG, ptr(x), ptr(y), B, hi, lo, None,
                                                    ptr(trail_s[k:]), ptr(trail_0[k:]), stream_ptr()))
            k += hi - lo + 1
        rec.update(x=sha(x), trail_sample=sha(trail_s), trail_x0=sha(trail_0))
        self.tail(rec, B, guided, d, y)
        return rec

    def known(self, d, method, eta, B, guided, segments, resample, given, seed):
        """latte_sample_loop_known over descending segments (hi ... lo each), the start blend in the first call only"""
        x, y = self.inputs(B, guided, seed)
        g = torch.Generator("cpu").manual_seed(seed + 100)
        half = B // 2 if guided else B
        known = torch.randn((half,) + self.shape, generator=g)
        mask = torch.zeros(half, self.shape[0], self.shape[2], self.shape[3])
        mask[:, 0] = 1.0                                             # the first frame, and a box in the others
        mask[:, 1:, 2:5, 3:7] = 1.0
        if guided:
            known, mask = torch.cat([known, known]), torch.cat([mask, mask])
        known, mask = known.cuda().contiguous(), mask.cuda().contiguous()
        self.m.set_engine_option("seed", seed, batch=B, guided=guided)
        eng, rec = self.m.engine(B, guided), {}
        name = "ddpm" if method == DDPM else "ddim"
        counts = [d.known_chain_slabs(name, eta, resample, hi, lo, j == 0) for j, (lo, hi) in enumerate(segments)]
        slabs = torch.randn((sum(counts),) + tuple(x.shape), generator=g).cuda() if given else None
        n = sum(hi - lo + 1 for lo, hi in segments)
        trail_s = torch.empty((n,) + tuple(x.shape), device="cuda")
        trail_0 = torch.empty_like(trail_s)
        k = taken = 0
        for j, (lo, hi) in enumerate(segments):
            nz = slabs[taken:taken + counts[j]].contiguous() if given and counts[j] else None
            check(self.lib.latte_sample_loop_known(eng, d._h, method, eta, 1, int(guided), CFG, ptr(x), ptr(y), B, hi, lo, ptr(known), ptr(mask),
                                                   resample, int(j == 0), ptr(nz), ptr(trail_s[k:]), ptr(trail_0[k:]), stream_ptr()))
            torch.cuda.synchronize()
            k += hi - lo + 1
            taken += counts[j]
        rec.update(x=sha(x), trail_sample=sha(trail_s), trail_x0=sha(trail_0), n_slabs=sum(counts))
        self.tail(rec, B, guided, d, y)
        return rec

    def front_end(self, d, loop, B, guided, seed):
        """A progressive loop of SpacedDiffusion on torch.manual_seed draws, three indices per engine call"""
        x, y = self.inputs(B, guided, seed)
        mk = {} if y is None else dict(y=y)
        if guided:
            mk["cfg_scale"] = CFG
        fn = self.m.forward_with_cfg if guided else self.m.forward
        torch.manual_seed(seed)
        per_index = x.numel() * 4
        if loop == "p_sample":
            it = d.p_sample_loop_progressive(fn, x.shape, x, model_kwargs=mk)
        elif loop == "ddim_reverse":
            it = d.ddim_reverse_sample_loop_progressive(fn, x, model_kwargs=mk)
        else:
            g = torch.Generator("cpu").manual_seed(seed + 100)
            known = torch.randn(tuple(x.shape), generator=g).cuda()
            mask = torch.zeros(B, self.shape[0], self.shape[2], self.shape[3], device="cuda")
            mask[:, 0] = 1.0
            if guided:
                known[B // 2:] = known[:B // 2]
            per_index *= 3 * 2
            it = d.known_sample_loop_progressive(fn, x.shape, known, mask, method="ddpm", noise=x, model_kwargs=mk, resample=2)
        d.SEGMENT_BYTES = 3 * per_index
        try:
            out = [(r["sample"].clone(), r["pred_xstart"].clone()) for r in it]
        finally:
            del d.SEGMENT_BYTES
        return {"n": len(out), "trail_sample": sha(torch.stack([a for a, _ in out])), "trail_x0": sha(torch.stack([b for _, b in out]))}

    def bpd(self, d, B, given, seed):
        x, y = self.inputs(B, False, seed)
        self.m.set_engine_option("seed", seed, batch=B)
        noise = None
        if given:
            noise = torch.randn((d.num_timesteps,) + tuple(x.shape), generator=torch.Generator("cpu").manual_seed(seed + 1)).cuda()
        out = d.calc_bpd_loop(self.m.forward, x, clip_denoised=True, model_kwargs={} if y is None else dict(y=y), noise=noise)
        rec = {k: sha(v) for k, v in out.items()}
        self.tail(rec, B, False, d, y)
        return rec

    def plan(self, d, method, B, guided, seed):
        x, y = self.inputs(B, guided, seed)
        self.m.set_engine_option("seed", seed, batch=B, guided=guided)
        mk = {} if y is None else dict(y=y)
        if guided:
            mk["cfg_scale"] = CFG
        fn = self.m.forward_with_cfg if guided else self.m.forward
        trail = [r["sample"] for r in d.linear_sample_loop_progressive(fn, x.shape, x, method=method, model_kwargs=mk)]
        rec = {"x": sha(trail[-1]), "trail_sample": sha(torch.stack(trail)), "n_evals": len(trail)}
        self.tail(rec, B, guided, d, y)
        return rec


def class_cases(out):
    d80, d10, d6, d40 = (latte_amd.create_diffusion(s) for s in ("80", "10", "6", "40"))
    cc, un = ClassEngine("tiny_classcond"), ClassEngine("tiny_uncond")
    whole, split = [(5, 74)], [(40, 74), (5, 39)]                 # 70 steps at bu = 4: two conditioning chunks
    for tag, method, eta in (("ddpm", DDPM, 0.0), ("ddim_eta0", DDIM, 0.0), ("ddim_eta0.5", DDIM, 0.5)):
        out[f"sample::{tag}::classcond::guided4::whole"] = cc.sample(d80, method, eta, 4, True, whole, 11)
        out[f"sample::{tag}::classcond::guided4::split"] = cc.sample(d80, method, eta, 4, True, split, 11)
        out[f"sample::{tag}::classcond::plain3"] = cc.sample(d10, method, eta, 3, False, [(0, 9)], 12)
        out[f"sample::{tag}::uncond::plain2"] = un.sample(d10, method, eta, 2, False, [(0, 9)], 13)
    out["invert::classcond::guided4::whole"] = cc.sample(d80, None, 0.0, 4, True, whole, 14, invert=True)
    out["invert::classcond::guided4::split"] = cc.sample(d80, None, 0.0, 4, True, [(5, 39), (40, 74)], 14, invert=True)
    out["invert::uncond::plain2"] = un.sample(d10, None, 0.0, 2, False, [(0, 9)], 15, invert=True)
    for e in (cc, un):
        for given in (True, False):
            out[f"bpd::{e.name}::{'given' if given else 'drawn'}"] = e.bpd(d10, 3, given, 16)
    for method in LINEAR:
        out[f"plan::{method}::classcond::guided4"] = cc.plan(d6, method, 4, True, 17)
        out[f"plan::{method}::classcond::plain3"] = cc.plan(d6, method, 3, False, 18)
        out[f"plan::{method}::uncond::plain2"] = un.plan(d6, method, 2, False, 19)
    out["plan::heun::classcond::guided4::40"] = cc.plan(d40, "heun", 4, True, 20)
    for tag, method, eta in (("ddpm", DDPM, 0.0), ("ddim_eta0", DDIM, 0.0), ("ddim_eta0.5", DDIM, 0.5)):
        for r in (1, 2):
            for given in (False, True):
                key = f"known::{tag}::resample{r}::{'given' if given else 'drawn'}"
                out[f"{key}::classcond::guided4::whole"] = cc.known(d80, method, eta, 4, True, whole, r, given, 22)
                out[f"{key}::classcond::guided4::split"] = cc.known(d80, method, eta, 4, True, split, r, given, 22)
                out[f"{key}::classcond::plain3"] = cc.known(d10, method, eta, 3, False, [(0, 9)], r, given, 23)
                out[f"{key}::uncond::plain2"] = un.known(d10, method, eta, 2, False, [(0, 9)], r, given, 24)
    for loop in ("p_sample", "ddim_reverse", "known"):
        out[f"front_end::{loop}::classcond::guided4"] = cc.front_end(d10, loop, 4, True, 25)
        out[f"front_end::{loop}::uncond::plain2"] = un.front_end(d10, loop, 2, False, 26)


def t2v_cases(out):
    from latte_amd.schedulers import (DDIMScheduler, DPMSolverMultistepScheduler, EulerAncestralDiscreteScheduler, EulerDiscreteScheduler,
                                      HeunDiscreteScheduler)
    z = np.load(os.path.join(ROOT, "tests", "golden", "tiny_t2v.npz"))
    cfg = json.loads(bytes(z["cfg_json"]).decode())
    sd = {k[4:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("sd::")}
    m = latte_amd.LatteT2V(num_attention_heads=cfg["num_attention_heads"], attention_head_dim=cfg["attention_head_dim"],
                           in_channels=cfg["in_channels"], out_channels=cfg["out_channels"], num_layers=cfg["num_layers"],
                           sample_size=cfg["sample_size"], patch_size=cfg["patch_size"], cross_attention_dim=cfg["cross_attention_dim"],
                           caption_channels=cfg["caption_channels"], video_length=cfg["video_length"], compute_dtype="f16", max_batch=4)
    m.load_state_dict(sd)
    pipe = latte_amd.LattePipeline(transformer=m, scheduler=DDIMScheduler()).to("cuda")
    g = torch.Generator("cpu").manual_seed(9)
    pe, ne = (torch.randn(2, 6, cfg["caption_channels"], generator=g) for _ in range(2))
    lat = torch.randn(2, 4, cfg["video_length"], cfg["sample_size"], cfg["sample_size"], generator=g)
    classes = {"ddim": DDIMScheduler, "euler": EulerDiscreteScheduler, "euler_a": EulerAncestralDiscreteScheduler,
               "heun": HeunDiscreteScheduler, "dpmsolver++": DPMSolverMultistepScheduler}
    for name, cls in classes.items():
        pipe.scheduler = cls()
        video = pipe(prompt_embeds=pe, negative_prompt_embeds=ne, num_inference_steps=6, guidance_scale=4.5, latents=lat,
                     generator=torch.Generator("cpu").manual_seed(21), output_type="latents").video
        out[f"t2v::{name}"] = {"latents": sha(video)}
    pipe.scheduler = DDIMScheduler()
    known = torch.randn(lat.shape, generator=g)
    mask = torch.zeros(2, cfg["video_length"], cfg["sample_size"], cfg["sample_size"])
    mask[:, 0] = 1.0
    video = pipe(prompt_embeds=pe, negative_prompt_embeds=ne, num_inference_steps=6, guidance_scale=4.5, latents=lat,
                 generator=torch.Generator("cpu").manual_seed(21), output_type="latents", known_latents=known, known_mask=mask).video
    out["t2v::ddim::known"] = {"latents": sha(video)}


def forward_cases(out):
    """One denoiser forward per case, at the width where the block's shape rules select every kernel: the rolling kernel, the 128 x 144 tile,
    split-K and the split operands of guided calls never run at the golden fixtures' D = 128."""
    from _util import engine_model, load_golden_model
    from latte_amd.random_init import randomize_zero_init, t2v_state_dict

    def xl(dtype, max_batch):
        torch.manual_seed(31)
        m = latte_amd.Latte(hidden_size=1152, num_heads=16, depth=2, patch_size=2, input_size=32, num_frames=16, num_classes=10, extras=2,
                            learn_sigma=True, compute_dtype=dtype, max_batch=max_batch)
        return randomize_zero_init(m, seed=32).cuda().eval()

    def inputs(B, guided):
        g = torch.Generator("cpu").manual_seed(33 + B + 100 * guided)
        half = B // 2 if guided else B
        x, t, y = torch.randn(half, 16, 4, 32, 32, generator=g), torch.randint(0, 1000, (half,), generator=g), torch.randint(0, 10, (half,), generator=g)
        if guided:
            x, t, y = torch.cat([x, x]), torch.cat([t, t]), torch.cat([y, torch.full_like(y, 10)])
        return x.cuda(), t.cuda(), y.cuda()

    def run(m, key, B, guided=False, **options):
        """the forward under `options`, which are put back to what they were behind it"""
        before = {k: m.get_engine_option(k, batch=B, guided=guided) for k in options}
        for k, v in options.items():
            m.set_engine_option(k, v, batch=B, guided=guided)
        x, t, y = inputs(B, guided)
        if guided:
            rec = {"out": sha(m.forward_with_cfg(x, t, y=y, cfg_scale=CFG))}
            rec["guided_split_active"] = m.get_engine_option("guided_split_active", batch=B, guided=True)
        else:
            rec = {"out": sha(m(x, t, y=y))}
        for k, v in before.items():
            m.set_engine_option(k, v, batch=B, guided=guided)
        out["forward::xl::" + key] = rec

    m = xl("f16", 8)
    for B in (1, 2, 8):
        run(m, f"B{B}", B)
    for v in (1, 2):
        run(m, f"B1::gated_split_k{v}", 1, gated_split_k=v)
    run(m, "B8::gated_rmw_shape0", 8, gated_rmw_shape=0)
    run(m, "B8::fc2_temp_embed0", 8, fc2_temp_embed=0)
    for v in (8, 11):
        run(m, f"B8::gemm_variant_fc2_{v}", 8, gemm_variant_fc2=v)
    for v in (0, 1, 2, 31):
        run(m, f"B8::fuse_qkv_attn{v}", 8, fuse_qkv_attn=v)
    for B in (2, 8):
        for v in (0, 3, 12, 20):
            run(m, f"cfg::B{B}::guided_split{v}", B, guided=True, guided_split=v)
    for v in (0, 15):          # last: once set, the option holds at every batch
        run(m, f"B8::stream_policy{v}", 8, stream_policy=v)
    del m
    m = xl("bf16", 2)
    run(m, "bf16::B2", 2)
    run(m, "bf16::cfg::B2", 2, guided=True)
    del m
    for name in ("tiny_classcond", "tiny_uncond", "tiny_textcond"):      # the un-fused flash path, extras == 78
        kw, sd, r = load_golden_model(name)
        m = engine_model(kw, sd, "f16", max_batch=4)
        mk = {k: torch.from_numpy(r[k]).cuda() for k in ("y", "text_embedding") if k in r}
        out[f"forward::{name}"] = {"out": sha(m(torch.from_numpy(r["x"]).cuda(), torch.from_numpy(r["t"]).cuda(), **mk))}
        if "x_cfg" in r:
            if "y_cfg" in r:
                mk["y"] = torch.from_numpy(r["y_cfg"]).cuda()
            xc = torch.from_numpy(r["x_cfg"]).cuda()
            tc = torch.from_numpy(r["t"]).cuda()[:1].expand(xc.shape[0]).contiguous()
            out[f"forward::{name}::cfg"] = {"out": sha(m.forward_with_cfg(xc, tc, cfg_scale=CFG, **mk)),
                                            "guided_split_active": m.get_engine_option("guided_split_active", batch=xc.shape[0], guided=True)}
        del m

    sd = t2v_state_dict(34, num_layers=1, caption_channels=128)
    g = torch.Generator("cpu").manual_seed(35)
    enc, mask = torch.randn(2, 20, 128, generator=g).cuda(), torch.ones(2, 20).cuda()
    mask[0, 12:] = 0
    mask[1, 17:] = 0
    for size, frames, variants in ((32, 16, [(temporal, fuse) for temporal in (True, False) for fuse in (0, 3)]), (64, 16, [(True, 3)]),
                                   (16, 1, [(True, 3)])):
        m = latte_amd.LatteT2V(num_attention_heads=16, attention_head_dim=72, num_layers=1, caption_channels=128, sample_size=size,
                               video_length=frames, compute_dtype="f16", max_batch=2).load_state_dict(sd).to("cuda")
        x, t = torch.randn(2, 4, frames, size, size, generator=g).cuda(), torch.tensor([500, 20]).cuda()
        m.set_text(enc, mask)                                            # an engine exists from here on (set_engine_option)
        for temporal, fuse in variants:
            m.set_engine_option("fuse_qkv_attn", fuse)
            o = m(x, t, enc, encoder_attention_mask=mask, enable_temporal_attentions=temporal).sample
            out[f"forward::t2v::size{size}::frames{frames}::temporal{int(temporal)}::fuse_qkv_attn{fuse}"] = {"out": sha(o)}
        del m


GROUPS = {"class": class_cases, "t2v": t2v_cases, "forward": forward_cases}


def compare(a, b):
    ra, rb = (json.load(open(p))["cases"] for p in (a, b))
    bad = sorted(k for k in set(ra) | set(rb) if ra.get(k) != rb.get(k))
    print(f"{len(ra)} / {len(rb)} cases, {len(bad)} differ" + "".join("\n  " + k for k in bad))
    return 1 if bad or not ra else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--compare", nargs=2, metavar="JSON")
    ap.add_argument("--tree", help="the built checkout to import latte_amd and tests/_util from (default: this one)")
    ap.add_argument("--only", choices=sorted(GROUPS), help="run this case group alone (default: all of them)")
    a = ap.parse_args()
    if a.compare:
        raise SystemExit(compare(*a.compare))
    if not torch.cuda.is_available():
        raise SystemExit("tools/chain_ab.py needs an MI355X")
    torch.set_grad_enabled(False)
    cases = {}
    for name, group in GROUPS.items():
        if a.only in (None, name):
            group(cases)
    result = {"what": "sha256 of every tensor the engine's fused loops return, fixed seeds (tools/chain_ab.py)",
              "library": "LATTE_AMD_LIB" if os.environ.get("LATTE_AMD_LIB") else "tree", "version": load_library().latte_version().decode(),
              "device": torch.cuda.get_device_name(0), "arch": torch.cuda.get_device_properties(0).gcnArchName, "cases": cases}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{len(cases)} cases -> {a.out}")


if __name__ == "__main__":
    main()
