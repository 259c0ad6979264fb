"""Host-side mirror of the reference interface (no GPU): registry, state_dict key set, config
loading, create_diffusion, and the product path refusing to run without its HIP backend."""
import os

import numpy as np
import pytest
import torch

import latte_amd
from _util import load_golden_model


def test_registry_has_the_twelve_presets():
    want = {f"Latte-{f}/{p}" for f in ("XL", "L", "B", "S") for p in (2, 4, 8)}
    assert set(latte_amd.Latte_models) == want                      # latte.py:501-506


def test_state_dict_keys_match_reference_checkpoint():
    for name in ("tiny_classcond", "tiny_uncond"):
        kw, sd, _ = load_golden_model(name)
        m = latte_amd.Latte(**kw)
        own = m.state_dict()
        assert set(own) == set(sd)
        for k in sd:
            assert tuple(own[k].shape) == tuple(sd[k].shape), k
        m.load_state_dict(sd, strict=True)
        # fixed sin-cos tables are rebuilt identically to the checkpoint's (latte.py:266-271)
        m2 = latte_amd.Latte(**kw)
        assert torch.equal(m2.pos_embed, sd["pos_embed"]) and torch.equal(m2.temp_embed, sd["temp_embed"])


def test_default_init_is_adaln_zero():
    m = latte_amd.Latte_models["Latte-S/2"](input_size=8, num_frames=4, num_classes=5, extras=2)
    assert float(m.blocks[0].adaLN_modulation[1].weight.abs().max()) == 0.0
    assert float(m.final_layer.linear.weight.abs().max()) == 0.0
    assert m.y_embedder.embedding_table.weight.shape == (6, 384)
    n = sum(p.numel() for p in latte_amd.Latte_models["Latte-S/2"](input_size=64, num_frames=4).parameters())
    assert abs(n / 1e6 - 32.9) < 0.2                                   # 32.9 M


def test_get_models_reads_reference_config_keys(tmp_path):
    y = tmp_path / "sample.yaml"
    y.write_text("ckpt:\nmodel: Latte-S/2\nnum_frames: 4\nimage_size: 64\nlearn_sigma: True\nextras: 2\n"
                 "num_classes: 101\nuse_fp16: True\nsample_method: 'ddpm'\nnum_sampling_steps: 250\ncfg_scale: 7.0\n"
                 "per_proc_batch_size: 2\nnum_fvd_samples: 2\n")
    cfg = latte_amd.load_config(str(y))
    cfg.ckpt = "x.pt"                                                   # sample.py:137
    cfg.latent_size = cfg.image_size // 8                               # sample.py:54-55
    assert cfg.ckpt == "x.pt" and cfg.cfg_scale == 7.0 and cfg.sample_method == "ddpm"
    m = latte_amd.get_models(cfg)
    assert m.input_size == 8 and m.extras == 2 and m.num_frames == 4
    cfg.model = "LatteIMG-XL/2"                                         # joint image-video training variant: not in the engine
    with pytest.raises(latte_amd.LatteError):
        latte_amd.get_models(cfg)
    cfg.model = "LatteT2V"                                              # dispatches to from_pretrained (tests/test_checkpoints.py)
    with pytest.raises(AttributeError):
        latte_amd.get_models(cfg)                                       # the reference's config needs pretrained_model_path too


def test_create_diffusion_surface(lib):
    d = latte_amd.create_diffusion("250")
    assert d.num_timesteps == 250 and d.timestep_map[:3] == [0, 4, 8] and d.timestep_map[-1] == 999
    assert abs(d.betas[-1] - 0.077519344992350026) < 1e-18
    assert abs(d.alphas_cumprod[-1] - 4.0358297653756747e-05) < 1e-19
    d = latte_amd.create_diffusion("")
    assert d.num_timesteps == 1000
    d = latte_amd.create_diffusion("250", learn_sigma=False, sigma_small=True, predict_xstart=True)   # init:32-45
    assert (d.learn_sigma, d.sigma_small, d.predict_xstart) == (False, True, True)
    with pytest.raises(latte_amd.LatteError):
        latte_amd.create_diffusion("ddim600")


@pytest.mark.skipif(torch.cuda.is_available(), reason="CPU-only behaviour")
def test_product_path_fails_loudly_without_gpu(lib):
    m = latte_amd.Latte_models["Latte-S/2"](input_size=8, num_frames=4)
    with pytest.raises(latte_amd.LatteError):
        m(torch.zeros(1, 4, 4, 8, 8), torch.zeros(1, dtype=torch.int64))
    d = latte_amd.create_diffusion("10")
    with pytest.raises(latte_amd.LatteError):
        d.ddim_sample_loop(m.forward, (1, 4, 4, 8, 8), torch.zeros(1, 4, 4, 8, 8), clip_denoised=False,
                           model_kwargs=dict(y=None), device="cpu")


def test_product_never_imports_the_oracle():
    import subprocess
    import sys
    code = "import sys, latte_amd; bad=[m for m in sys.modules if m.split('.')[0]=='oracle']; assert not bad, bad"
    subprocess.run([sys.executable, "-c", code], check=True,
                   cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    root = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "latte_amd")
    for dirpath, _, files in os.walk(root):
        for f in files:
            if f.endswith((".py", ".hip", ".cpp", ".h")):
                src = open(os.path.join(dirpath, f)).read()
                assert "import oracle" not in src and "from oracle" not in src, f


def test_half_dtype_selects_engine_operand_type():
    """sample.py:72-75: model.to(dtype=torch.float16) under use_fp16 -> f16 MFMA operands, fp32 master weights."""
    import torch
    from latte_amd.models import Latte_models
    m = Latte_models["Latte-S/2"](input_size=8, num_frames=4, extras=1)
    # nothing pinned: f16 operands for every call (round 4: the type that holds 1e-3 at trained-checkpoint gate magnitudes)
    assert m.compute_dtype is None and m.operand_dtype() == "f16" and m.operand_dtype(guided=True) == "f16"
    m.to(dtype=torch.float16)
    assert m.operand_dtype() == m.operand_dtype(guided=True) == "f16"
    assert m.compute_dtype == "f16" and m.pos_embed.dtype == torch.float32
    m.to(torch.bfloat16)
    assert m.compute_dtype == "bf16" and m.operand_dtype(guided=True) == "bf16"      # pinned for every call


def test_avi_round_trip(tmp_path):
    """Video hand-off (sample.py:124-126 writes .mp4 through imageio; offline: uncompressed AVI): header fields and every
    frame survive a write / read round trip, including a width whose rows need DIB padding."""
    import numpy as np
    from latte_amd import read_avi, write_avi
    for shape in [(4, 8, 8, 3), (3, 6, 7, 3), (16, 32, 30, 3)]:
        v = np.random.default_rng(sum(shape)).integers(0, 256, shape, dtype=np.uint8)
        path = str(tmp_path / "v.avi")
        write_avi(path, torch.from_numpy(v), fps=8)
        back, fps = read_avi(path)
        assert fps == 8.0 and np.array_equal(back, v)
        raw = open(path, "rb").read()
        assert raw[:4] == b"RIFF" and raw[8:12] == b"AVI " and int.from_bytes(raw[4:8], "little") == len(raw) - 8
    with pytest.raises(ValueError):
        write_avi(str(tmp_path / "bad.avi"), np.zeros((2, 4, 4), dtype=np.uint8))


def test_mp4_round_trip(tmp_path):
    """The reference's hand-off is an .mp4 (sample.py:123-126, sample_ddp.py:174-176).  write_mp4 puts Motion-JPEG samples into an
    ISO base-media file: box structure (ftyp first, one mdat, one moov with a single video track whose sample table addresses
    every frame), frame count / size / rate, and the decoded frames within JPEG tolerance of the uint8 input."""
    import struct
    import numpy as np
    from latte_amd import read_mp4, write_mp4
    f, h, w = 16, 64, 96
    yy, xx = np.mgrid[0:h, 0:w]
    v = np.stack([np.stack([127 + 100 * np.sin(xx / 9 + i / 3), 127 + 100 * np.cos(yy / 7 - i / 5), (xx + yy + 4 * i) % 256], -1)
                  for i in range(f)]).astype(np.uint8)
    path = str(tmp_path / "v.mp4")
    write_mp4(path, torch.from_numpy(v), fps=8)
    raw = open(path, "rb").read()
    boxes, p = [], 0
    while p < len(raw):
        n, kind = struct.unpack_from(">I4s", raw, p)
        boxes.append((kind, p, n))
        p += n
    assert p == len(raw) and [b[0] for b in boxes] == [b"ftyp", b"mdat", b"moov"]
    assert raw[8:12] == b"isom" and b"mp4v" in raw and b"esds" in raw and raw.count(b"trak") == 1
    stco = raw.index(b"stco")
    assert struct.unpack_from(">I", raw, stco + 12)[0] == boxes[1][1] + 8        # the chunk offset points at the first JPEG
    assert raw[boxes[1][1] + 8: boxes[1][1] + 10] == b"\xff\xd8"                 # ... which starts with SOI
    back, fps = read_mp4(path)
    assert fps == 8.0 and back.shape == v.shape and back.dtype == np.uint8
    rms = float(np.sqrt(((back.astype(np.float64) - v) ** 2).mean()))
    assert rms < 2.5, rms
    for shape, rate in [((1, 5, 7, 3), 8), ((3, 33, 17, 3), 23.976), ((2, 256, 256, 3), 30)]:   # one frame, odd sizes, fractional rate
        u = np.random.default_rng(sum(shape)).integers(0, 256, shape, dtype=np.uint8)
        write_mp4(path, u, fps=rate)
        back, fps = read_mp4(path)
        assert back.shape == u.shape and abs(fps - rate) < 1e-9
    with pytest.raises(ValueError):
        write_mp4(str(tmp_path / "bad.mp4"), np.zeros((2, 4, 4), dtype=np.uint8))


def test_oracle_is_only_imported_by_the_checkers():
    """The oracle is test infrastructure: only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg may import it.
    The package, the tools and the rest of bench.py must not (random weights for plumbing runs come from
    latte_amd.random_init)."""
    import ast
    import glob
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

    def oracle_imports(path):
        hits = []
        tree = ast.parse(open(path).read())
        for fn in [n for n in ast.walk(tree) if isinstance(n, (ast.FunctionDef, ast.Module))]:
            for n in ast.iter_child_nodes(fn) if isinstance(fn, ast.Module) else ast.walk(fn):
                if isinstance(n, ast.ImportFrom) and (n.module or "").split(".")[0] == "oracle":
                    hits.append(fn.name if isinstance(fn, ast.FunctionDef) else "<module>")
                if isinstance(n, ast.Import) and any(a.name.split(".")[0] == "oracle" for a in n.names):
                    hits.append(fn.name if isinstance(fn, ast.FunctionDef) else "<module>")
        return hits

    for path in glob.glob(os.path.join(root, "latte_amd", "*.py")) + glob.glob(os.path.join(root, "tools", "*.py")):
        assert oracle_imports(path) == [], path
    assert set(oracle_imports(os.path.join(root, "bench.py"))) <= {"cpu_baseline"}
    assert set(oracle_imports(os.path.join(root, "__graft_entry__.py"))) <= {"smoke"}


def test_bench_reads_power_and_clock_from_rocm_smi_json():
    """bench.py's power_check samples `rocm-smi -c -P --json`; the text below is what the tool prints on the GPU boxes of the pool
    (profiles/r4_operand_power_probe_gemm.log, last line).  Unreadable output must give (None, None), never an exception."""
    import importlib.util
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("bench_for_test", os.path.join(root, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    txt = ('{"card0": {"fclk clock speed:": "(1250Mhz)", "fclk clock level:": "0", "mclk clock speed:": "(2000Mhz)", '
           '"mclk clock level:": "0", "sclk clock speed:": "(2403Mhz)", "sclk clock level:": "1", "socclk clock speed:": "(73Mhz)", '
           '"socclk clock level:": "S", "Current Socket Graphics Package Power (W)": "771.0"}}')
    assert bench.parse_rocm_smi(txt) == (771.0, 2403.0)
    assert bench.parse_rocm_smi("") == (None, None)
    assert bench.parse_rocm_smi('{"card0": {"sclk clock speed:": "n/a"}}') == (None, None)
    one = lambda w, mhz: '{"card0": {"sclk clock speed:": "(%dMhz)", "Current Socket Graphics Package Power (W)": "%.1f"}}' % (mhz, w)  # noqa: E731
    samples = [(10.0, one(700, 2400)), (10.2, one(900, 2300)), (10.4, one(1390, 1700)), (11.0, one(1400, 1710)), (11.2, "garbage"),
               (12.5, one(800, 2400))]
    assert bench.mean_power_clock(samples, 10.0, 12.0) == (1395.0, 1705.0, 2)      # the first 0.3 s and everything after b are left out
    assert bench.mean_power_clock([], 0.0, 1.0) == (None, None, 0)


def test_bench_energy_columns_are_power_times_time():
    """bench.py: energy = the forward leg's mean socket power x this run's times (round-4 review: the quantity the power-capped MFMA
    kernels are bound by); no power sample -> no energy object, the line still prints."""
    import bench
    res = {"ms_per_step": 30.0, "config": {"per_gpu_batch": 8},
           "roofline_table": [{"class": "gemm_fc2", "avg_launch_ms": 0.3}, {"class": "ln_modulate", "avg_launch_ms": 0.04}],
           "power_check": {"forward": {"socket_power_w": 1350.0, "shader_clock_mhz": 1920.0},
                           "fc2_standalone_random_operands": {"socket_power_w": 1390.0, "avg_launch_ms": 0.3117},
                           "fc2_standalone_zeros_operands": {"socket_power_w": 1119.0, "avg_launch_ms": 0.2495}}}
    en = bench.energy_columns(res, 1)
    assert en["joules_per_step"] == 40.5 and en["joules_per_sample_step"] == round(40.5 / 8, 3)
    assert abs(en["picojoules_per_algorithmic_flop"] - 40.5 / 8 / 3.726e12 * 1e12) < 2e-3
    assert res["roofline_table"][0]["joules_per_launch"] == 0.405 and res["roofline_table"][1]["joules_per_launch"] == 0.054
    assert res["power_check"]["fc2_standalone_random_operands"]["joules_per_launch"] == round(1390.0 * 0.3117e-3, 4)
    assert bench.energy_columns({"power_check": {"error": "no rocm-smi"}, "ms_per_step": 1.0, "config": {"per_gpu_batch": 8}}, 1) is None


def test_bench_vae_conv_algorithmic_bytes():
    """bench.py: the convolutions of a 16-frame SD-VAE decode move 14.4 GB algorithmically (operand in, fp32 out, fp32 residual, weights
    once) -- the figure the round-4 review asked for beside the 24.4 GB of fabric traffic the PMC pass counts."""
    import bench
    b = bench.vae_conv_bytes(32)
    assert 14.3e9 < b < 14.5e9
    assert bench.vae_conv_bytes(32, frames=1) < b / 14          # the weights (96 MB) are read once per decode, not per frame


def test_bench_dump_outputs_full_or_fixed_sample(tmp_path, monkeypatch):
    """bench.py --dump-outputs: the timed path's result in fp32, whole while it fits its rank's share of DUMP_BYTES, otherwise the same
    seeded sample of its elements in every run."""
    import bench
    t = torch.randn(2, 3, 4, 5, dtype=torch.float64)
    bench.dump_outputs(str(tmp_path / "a"), "samples", t, 1)
    got = np.load(tmp_path / "a" / "samples.npy")
    assert got.dtype == np.float32 and got.shape == (2, 3, 4, 5) and np.array_equal(got, t.float().numpy())
    monkeypatch.setattr(bench, "DUMP_BYTES", 4 * 40)
    for d in ("b", "c"):
        bench.dump_outputs(str(tmp_path / d), "samples_rank1", t, 2)
    s = np.load(tmp_path / "b" / "samples_rank1.npy")
    assert s.shape == (20,) and np.array_equal(s, np.load(tmp_path / "c" / "samples_rank1.npy"))
    assert np.isin(s, t.float().numpy().reshape(-1)).all() and len(np.unique(s)) == 20
