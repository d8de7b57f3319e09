"""CPU: host logic of the drop-in boundary -- the C ABI library loads and exports every declared symbol, argument
validation works without a GPU, the `src.models.*` classes keep the reference's constructor / state-dict contract and
fail loudly (no fallback) off the HIP device or in grad mode."""
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class Conf:
    def __init__(self, module=None, kwargs=None):
        self.module, self.kwargs = module, (kwargs or {})


def build_nerf():
    from src.util.import_helper import import_obj
    return import_obj("src.models.pixelnerf.PixelNeRF")(
        poscode_conf=Conf(kwargs=dict(num_freqs=6, freq_factor=6.28, include_input=True)),
        encoder_conf=Conf("src.models.image_encoder.SpatialEncoder", dict(image_padding=64, padding_pe=4, pretrained=False)),
        mlp_fine_conf=Conf("src.models.resnetfc.ResnetFC", dict(n_blocks=5, d_hidden=512, combine_layer=3,
                                                                 combine_type="average")))


def test_training_workspace_split_is_consistent():
    """Host arithmetic only (no device work): the two parts of the training workspace (round 5: what the forward keeps for the backward, per
    object / the work buffers the objects of a step share) add up to the one-buffer size of the older entry points, for the shipped step, the
    reference batch and ragged sizes; the saved part is what autograd holds per object (10.84 GiB at 4096 rays x 40 samples x 4 views)."""
    import ctypes as C
    from diner_amd import _lib
    lib = _lib.load()
    for P, nv in ((163840, 4), (5120, 4), (200, 4), (1, 4), (4097, 3)):
        a, b = C.c_size_t(0), C.c_size_t(0)
        assert lib.diner_field_train_workspace_split(P, nv, C.byref(a), C.byref(b)) == 0
        assert a.value > 0 and b.value > 0 and a.value % 256 == 0 and b.value % 256 == 0
        assert a.value + b.value == lib.diner_field_train_workspace_bytes(P, nv)
    lib.diner_field_train_workspace_split(163840, 4, C.byref(a), C.byref(b))
    assert 10.5 < a.value / 2 ** 30 < 11.0 and 4.4 < b.value / 2 ** 30 < 4.7
    assert lib.diner_field_train_workspace_split(0, 4, C.byref(a), C.byref(b)) != 0      # bad sizes are an error, not a zero


def test_library_exports_every_declared_symbol():
    import ctypes
    from diner_amd import _lib
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "diner_hip.h")).read()
    declared = set(re.findall(r"\b(diner_[a-z0-9_]+)\s*\(", header))
    assert declared, "no declarations found in include/diner_hip.h"
    for name in declared:
        assert hasattr(lib, name), f"libdiner_hip.so does not export {name}"
    assert declared == set(_lib.SIGNATURES), "ctypes SIGNATURES out of sync with include/diner_hip.h"
    assert lib.diner_abi_version() == _lib.ABI_VERSION == 6
    assert isinstance(lib.diner_last_error(), bytes)


def test_argument_validation_without_gpu():
    import ctypes as C
    from diner_amd import _lib
    lib = _lib.load()
    # null scene / bad sizes are rejected before any device call
    rc = lib.diner_sample_depthguided_f32(None, None, 0, 1000, 64, 24, 0.05, None, None, None, None, 0, 0, None, None, None)
    assert rc == -1 and b"null" in lib.diner_last_error()
    rc = lib.diner_composite_f32(C.c_void_p(8), C.c_void_p(8), C.c_void_p(8), 4, 1000, 0, C.c_void_p(8), C.c_void_p(8),
                                 None, None)
    assert rc == -1 and b"K" in lib.diner_last_error()
    # configurations outside what the kernels are built for are refused by the C ABI itself, before any device work
    dummy = (C.c_float * 4)()
    arr = (C.c_void_p * 5)(*[C.addressof(dummy)] * 5)

    def params(**kw):
        p = _lib.DinerMlpParams()
        p.d_in, p.d_latent, p.d_hidden, p.d_out, p.n_blocks, p.combine_layer = 55, 512, 512, 4, 5, 3
        p.num_freqs, p.include_input, p.freq_factor = 6, 1, 6.28
        p.lin_in_w = p.lin_in_b = p.lin_out_w = p.lin_out_b = C.addressof(dummy)
        for f in ("fc0_w", "fc0_b", "fc1_w", "fc1_b", "lin_z_w", "lin_z_b"):
            setattr(p, f, C.cast(arr, C.POINTER(C.c_void_p)))
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    h = C.c_void_p()
    for bad, word in ((dict(d_hidden=128), b"ResnetFC"), (dict(freq_factor=1000.0), b"freq_factor"),
                      (dict(freq_factor=-6.28), b"freq_factor"), (dict(freq_factor=float("nan")), b"freq_factor"),
                      (dict(num_freqs=10), b"num_freqs"), (dict(include_input=0), b"include_input")):
        p = params(**bad)
        rc = lib.diner_mlp_create(C.byref(p), None, C.byref(h))
        assert rc == -2 and b"unsupported" in lib.diner_last_error() and word in lib.diner_last_error(), (bad, lib.diner_last_error())
        assert not h.value
    with pytest.raises(RuntimeError, match="unsupported"):
        _lib.check(rc)
    assert lib.diner_field_workspace_bytes(16) == 16 * 512 * 4 + 256    # 2 KB / point + the overflow flag
    assert lib.diner_field_workspace_bytes(17) == 32 * 512 * 4 + 256    # whole 16-point tiles
    # the arithmetic mode is a per-call argument: an unknown one is an argument error, and there is no global switch
    assert not hasattr(lib, "diner_set_precision") and not hasattr(lib, "diner_get_precision")
    fields = dict(_lib.DinerScene._fields_)
    assert {"poses_host", "focal_host", "c_host"} <= set(fields) and not {"poses", "focal", "c"} & set(fields)


def test_state_dict_contract():
    nerf = build_nerf()
    sd = nerf.state_dict()
    mlp = {k: tuple(v.shape) for k, v in sd.items() if k.startswith("mlp_fine.")}
    assert mlp["mlp_fine.lin_in.weight"] == (512, 55) and mlp["mlp_fine.lin_out.weight"] == (4, 512)
    assert all(mlp[f"mlp_fine.blocks.{b}.fc_{j}.weight"] == (512, 512) for b in range(5) for j in (0, 1))
    assert all(mlp[f"mlp_fine.lin_z.{b}.weight"] == (512, 512) for b in range(3)) and "mlp_fine.lin_z.3.weight" not in mlp
    assert sum(v.numel() for k, v in sd.items() if k.startswith("mlp_fine.")) == 3445252
    for k in ("poscode._freqs", "poscode._phases", "depthcode._freqs", "depthcode._phases",
              "encoder.positional_encoding._freqs", "encoder.positional_encoding._phases"):
        assert k in sd
    assert tuple(sd["encoder.model.conv1.weight"].shape) == (64, 21, 7, 7)     # 3 rgb + 18 padding-PE channels
    enc = [k for k in sd if k.startswith("encoder.model.")]
    assert len(enc) == 216                                                      # torchvision resnet34 minus fc
    assert "encoder.model.layer4.2.bn2.running_var" in sd and "encoder.model.layer2.0.downsample.1.weight" in sd
    # non-persistent buffers stay out of checkpoints
    assert "poses" not in sd and "encoder.latent" not in sd
    assert nerf.d_in == 55 and nerf.d_latent == 512 and nerf.d_out == 4
    # default init zeroes fc_1 like the reference (resnetfc.py:47)
    assert float(sd["mlp_fine.blocks.0.fc_1.weight"].abs().max()) == 0.0


def test_state_dict_matches_imported_reference():
    """Against the imported reference's state dict, stored by oracle/make_golden_state_dict.py (G21): every entry outside the
    ResNet trunk (a torchvision stub in the reference import) with its shape, and the positional-encoding buffers' values."""
    ref = np.load(os.path.join(ROOT, "tests", "golden", "g21_reference_state_dict.npz"), allow_pickle=False)
    shapes = {k[len("shape:"):]: tuple(int(x) for x in ref[k]) for k in ref.files if k.startswith("shape:")}
    values = {k[len("value:"):]: torch.from_numpy(ref[k]) for k in ref.files if k.startswith("value:")}
    assert len(shapes) == 36 and set(values) == {"poscode._freqs", "poscode._phases", "depthcode._freqs"}
    mine = build_nerf().state_dict()
    for k, shape in shapes.items():
        assert k in mine and tuple(mine[k].shape) == shape, k
    for k, v in values.items():
        assert torch.equal(mine[k], v)


def test_renderer_contract_and_no_fallback():
    from src.util.import_helper import import_obj
    R = import_obj("src.models.nerf_renderer.NeRFRendererDGS")
    r = R(n_samples=40, n_depth_candidates=1000, n_gaussian=15, white_bkgd=False)
    assert (r.n_samples, r.n_depth_candidates, r.n_gaussian, r.eval_batch_size, r.white_bkgd) == (40, 1000, 15, 100000, False)
    r.n_samples, r.n_gaussian = 128, int(15 * 128 / 40)         # create_prediction_folder.py:44-47 mutates these
    assert r.n_gaussian == 48
    nerf = build_nerf()
    rays = torch.zeros(1, 8, 8)
    with torch.no_grad():
        with pytest.raises((RuntimeError, AttributeError)):     # CPU tensors: no silent CPU path
            r.forward(nerf, rays)
        with pytest.raises(TypeError):
            r.forward(object(), rays)
        with pytest.raises(RuntimeError, match="HIP device"):
            nerf.poscode(torch.zeros(4, 3))
    with pytest.raises(RuntimeError, match="HIP device"):   # round 6: the explicit-matrix entry is differentiable (generic path) -- on the device only
        nerf.mlp_fine(torch.zeros(1, 4, 8, 567), combine_dim=1)
    z = r.sample_coarse(torch.tensor([[[0., 0, 0, 0, 0, 1, 0.5, 1.5]]]), 10)
    assert z.shape == (1, 1, 10) and bool(((z >= 0.5) & (z <= 1.5)).all())


def test_configurations_outside_the_fused_kernels_are_routed_to_the_generic_path():
    """Round 5: only the shipped configuration (55 / 512 / 512 / 4, 5 blocks, combine 3, NV 4, poscode 6 + input, ReLU) takes the fused
    kernels; the reference's constructor defaults and every other variation are classified for the generic slow path (csrc/generic.hip) --
    no configuration the reference accepts is refused any more (GPU parity: tests/test_generic_gpu.py)."""
    from src.models.resnetfc import ResnetFC
    shipped = ResnetFC(d_in=55, d_latent=512, n_blocks=5, d_hidden=512, combine_layer=3)
    assert shipped.is_fused_shape() and shipped.is_fused_shape(nv=4, num_freqs=6, include_input=True)
    assert not shipped.is_fused_shape(nv=3) and not shipped.is_fused_shape(num_freqs=4) and not shipped.is_fused_shape(include_input=False)
    for kw in (dict(d_in=55, d_latent=512), dict(d_in=55, d_latent=512, d_hidden=512, n_blocks=5, combine_layer=2),
               dict(d_in=55, d_latent=512, d_hidden=512, n_blocks=4, combine_layer=3), dict(d_in=55, d_latent=512, d_hidden=512, n_blocks=5, combine_layer=3, beta=1.0),
               dict(d_in=39, d_latent=512, d_hidden=512, n_blocks=5, combine_layer=3), dict(d_in=55, d_latent=0, d_hidden=512, n_blocks=5, combine_layer=3)):
        assert not ResnetFC(**kw).is_fused_shape(), kw
    with pytest.raises(NotImplementedError):
        ResnetFC(d_in=55, d_latent=512, combine_type="max")._check_supported()
    from diner_amd import _lib
    lib = _lib.load()
    for sym in ("diner_mlp_generic_forward_f32", "diner_mlp_generic_workspace_bytes", "diner_field_inputs_generic_f32"):
        assert hasattr(lib, sym)
    assert lib.diner_mlp_generic_workspace_bytes(None, 4, 10) == 0          # argument validation without a device


def test_shard_range_partition():
    from diner_amd.render import shard_range
    for n in (1, 7, 120000, 480000):
        for world in (1, 2, 3, 8):
            spans = [shard_range(n, r, world) for r in range(world)]
            assert spans[0][0] == 0 and spans[-1][1] == n
            assert all(spans[i][1] == spans[i + 1][0] for i in range(world - 1))
            assert max(h - l for l, h in spans) - min(h - l for l, h in spans) <= (n + world - 1) // world


def test_no_spill_code_inside_nsplit_gemms(tmp_path):
    """Codegen guard for the default per-view kernel (k_field_pre_h3n): no scratch (register spill) traffic between its
    first and last MFMA.  Builds of this kernel that spilled accumulators inside the GEMM loops returned wrong sums on
    the GPU for every tile after a workgroup's first one ('n-split kernel'); the resident version must stay
    spill-free there, so a compiler or source change that reintroduces such spills fails here, on the CPU box."""
    import re
    import shutil
    import subprocess
    from diner_amd import build as B
    hipcc = B._hipcc()
    if not (hipcc and (shutil.which(hipcc) or os.path.exists(hipcc))):
        pytest.skip("hipcc not available")
    out = tmp_path / "mlp_h3n.s"
    subprocess.check_call([hipcc] + B.FLAGS + ["-x", "hip", "-S", "--cuda-device-only",
                                                os.path.join(B.CSRC, "mlp_h3n.hip"), "-o", str(out)],
                          stderr=subprocess.DEVNULL)
    txt = out.read_text()
    pre = list(re.finditer(r"^(\w*k_field_pre_h3n\w*):.*?\n(.*?)\.Lfunc_end", txt, re.S | re.M))
    post = list(re.finditer(r"^(\w*k_field_post_h3n\w*):.*?\n(.*?)\.Lfunc_end", txt, re.S | re.M))
    assert len(pre) == 1 and len(post) == 1, "expected the one (f16x3) instance of each kernel"
    for m in pre:
        body = m.group(2).split("\n")
        idx = [i for i, l in enumerate(body) if "v_mfma" in l]
        assert len(idx) > 1500
        spills = [l for l in body[idx[0]:idx[-1] + 1] if "scratch_" in l]
        assert not spills, f"{m.group(1)}: {len(spills)} scratch accesses inside the GEMM span, e.g. {spills[:3]}"
        # round 3: the kernel has no scratch access at all (the own-chunk conversion reads accumulators through explicit
        # v_accvgpr_read with an "a" constraint; a plain read made the allocator spill accumulator tuples around the GEMMs)
        assert not [l for l in body if "scratch_" in l], m.group(1)
        assert any("v_cvt_pk_f16_f32" in l for l in body)
        assert any("v_fma_mix_f32" in l for l in body)      # the residual of the hi / lo split comes from v_fma_mix_f32 reading the fp16 half in place
        # second guard (round 2c): no packed-fp32 arithmetic between MFMAs.  v_pk_mul_f32 / v_pk_add_f32 / v_pk_fma_f32 do not
        # overlap with the wave's MFMAs (each costs a whole MFMA slot, tools/ubench/mfma_valu.hip); the in-GEMM gather blend is
        # written in single-width instructions for that reason, and a change that lets the compiler re-vectorise it shows up here
        packed = [i for i, l in enumerate(body) if re.match(r"\s*v_pk_(mul|add|fma)_f32", l)]
        import bisect
        inside = [i for i in packed if 0 < bisect.bisect(idx, i) < len(idx)
                  and i - idx[bisect.bisect(idx, i) - 1] < 30 and idx[bisect.bisect(idx, i)] - i < 30]
        assert len(inside) <= 16, f"{m.group(1)}: {len(inside)} packed-fp32 instructions inside MFMA streams (round 2c start: ~450)"
    # the post kernel (blocks 3-4 + lin_out on the vector ALU): no scratch between its first and last MFMA (an optimiser that sinks the
    # accumulation chains below the operand loads shows up as spills there).  It uses all 512 registers inside the GEMMs, so the tile
    # queue's thread-0 state (the next tile, requested at the top of a tile and handed over at the bottom) crosses them through scratch:
    # a handful of accesses per tile, outside the MFMA span
    for m in post:
        body = m.group(2).split("\n")
        idx = [i for i, l in enumerate(body) if "v_mfma" in l]
        assert len(idx) > 1000
        assert not [l for l in body[idx[0]:idx[-1] + 1] if "scratch_" in l], m.group(1)
        assert len([l for l in body if "scratch_" in l]) <= 16, m.group(1)


def test_eight_wave_kernels_codegen(tmp_path):
    """Round 5: the eight-wave per-view kernels (two waves per SIMD, 256 registers each; csrc/mlp_h3n.hip namespace w8).  A spill reload is a
    scratch LOAD, and loads return in order: one reload inside a GEMM waits for every weight fragment and tap in flight (the first version
    kept the hidden block alive across the gather-carrying GEMM, spilled 8 accumulator tuples inside it and ran 13 % slower than the
    four-wave kernel, profiles/r05_f16_w8_ab_runs.txt).  Pinned: the per-view kernel has at most 2 scratch accesses between its first and
    last MFMA, the post kernel none; both use the 16 x 16 x 32 fp16 MFMA and buffer loads for the weight ring."""
    import re
    import shutil
    import subprocess
    from diner_amd import build as B
    hipcc = B._hipcc()
    if not (hipcc and (shutil.which(hipcc) or os.path.exists(hipcc))):
        pytest.skip("hipcc not available")
    out = tmp_path / "mlp_h3n.s"
    subprocess.check_call([hipcc] + B.FLAGS + ["-x", "hip", "-S", "--cuda-device-only", os.path.join(B.CSRC, "mlp_h3n.hip"), "-o", str(out)],
                          stderr=subprocess.DEVNULL)
    txt = out.read_text()
    for name, n_mfma, max_inside in (("k_field_pre_h8", 1056, 2), ("k_field_post_h8", 512, 0)):
        m = re.search(r"^(\w*\d" + name + r"E\w*):.*?\n(.*?)\.Lfunc_end", txt, re.S | re.M)
        assert m, name
        body = m.group(2).split("\n")
        idx = [i for i, l in enumerate(body) if "v_mfma_f32_16x16x32_f16" in l]
        assert len(idx) == n_mfma, (name, len(idx))
        inside = [l for l in body[idx[0]:idx[-1] + 1] if "scratch_" in l]
        assert len(inside) <= max_inside, (name, len(inside))
        assert sum("buffer_load_dwordx4" in l for l in body) >= 100, name
        meta = re.search(r"\.amdhsa_kernel " + re.escape(m.group(1)) + r"(.*?)\.end_amdhsa_kernel", txt, re.S).group(1)
        assert int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", meta).group(1)) <= 256, name      # two waves per SIMD


def test_no_spill_code_in_the_training_kernels(tmp_path):
    """Codegen guard for the 512 x 512 layer products of the training path (csrc/train_512.hip): k_run512 (three tile shapes of the bf16x6
    forward / data-gradient body + the weight-gradient body in one kernel, one wave per SIMD at 496 registers), k_fwd512_f16x3 and k_run512_f16x3 carry no
    scratch access at all, and their MFMAs are the 32 x 32 x 16 ones of the arithmetic they claim."""
    import re
    import shutil
    import subprocess
    from diner_amd import build as B
    hipcc = B._hipcc()
    if not (hipcc and (shutil.which(hipcc) or os.path.exists(hipcc))):
        pytest.skip("hipcc not available")
    out = tmp_path / "train_512.s"
    subprocess.check_call([hipcc] + B.FLAGS + ["-x", "hip", "-S", "--cuda-device-only",
                                                os.path.join(B.CSRC, "train_512.hip"), "-o", str(out)],
                          stderr=subprocess.DEVNULL)
    txt = out.read_text()
    found = {}
    for name in ("k_run512", "k_fwd512_f16x3", "k_run512_f16x3"):
        m = re.search(r"^(\w*\d" + name + r"E\w*):.*?\n(.*?)\.Lfunc_end", txt, re.S | re.M)      # (Itanium mangling: <length><name>E...)
        assert m, name
        body = m.group(2).split("\n")
        spills = [l for l in body if "scratch_" in l]
        if name == "k_run512":
            assert not spills, name
        else:
            # round 4: the 128-row shape of the f16x3 bodies (256 accumulator registers) keeps ~10 loop-invariant scalars-in-VGPRs (row
            # strides, epilogue pointers) in scratch: stored once in front of the tile loop, reloaded in the epilogue -- none of it inside the
            # slab loop (no spill / reload is interleaved with MFMAs).  Bounded here.
            # round 5: the counts are pinned -- 40 / 54 with hipcc of ROCm 7.2 (35 / 49 before the bit-mask branch of the epilogue,
            # which keeps one more pointer) -- so that drift is visible
            assert len(spills) <= {"k_fwd512_f16x3": 6, "k_run512_f16x3": 18}[name], (name, len(spills))      # round 6 (epilogue of the 128-row shape through LDS, compile-time term sets): 0 / 12
            for i, l in enumerate(body):
                if "scratch_" in l:      # not interleaved with MFMAs: none within 25 instructions on BOTH sides
                    before = any("v_mfma" in x for x in body[max(0, i - 25):i])
                    after = any("v_mfma" in x for x in body[i + 1:i + 26])
                    assert not (before and after), f"{name}: scratch access among MFMAs: {l.strip()}"
        found[name] = body
    # round 5: the eight-wave weight gradient (two waves per SIMD: 256 registers, 128 of them accumulators) -- no scratch access inside its slab loop
    m = re.search(r"^(\w*\dk_wgrad512_w8E\w*):.*?\n(.*?)\.Lfunc_end", txt, re.S | re.M)
    assert m, "k_wgrad512_w8"
    body = m.group(2).split("\n")
    idx = [i for i, l in enumerate(body) if "v_mfma_f32_32x32x16_f16" in l]
    assert len(idx) == 48, len(idx)
    assert not [l for l in body[idx[0]:idx[-1] + 1] if "scratch_" in l]
    assert len([l for l in body if "scratch_" in l]) <= 15
    assert re.search(r"\.amdhsa_kernel \S*k_wgrad512_w8\S*\n.*?\.amdhsa_next_free_vgpr (\d+)", txt, re.S).group(1) == "256"
    assert sum("v_mfma_f32_32x32x16_bf16" in l for l in found["k_run512"]) > 1000
    assert sum("v_mfma_f32_32x32x16_f16" in l for l in found["k_fwd512_f16x3"]) > 500
    assert not any("v_mfma_f32_32x32x16_bf16" in l for l in found["k_fwd512_f16x3"])
    # round 4: the backward's launch in the f16x3 arithmetic: the data gradient in its four shapes.  The bound is a recount: the listing of
    # the commit before the kernel lost its weight-gradient tail had 1584 of these MFMAs, 144 of them in the tail that no launch reached
    # (96 in the four-wave 256 x 256-tile body, 48 in the f16x3 instance of the 128 x 256-tile body): 1584 - 144 = 1440
    assert sum("v_mfma_f32_32x32x16_f16" in l for l in found["k_run512_f16x3"]) >= 1440
    assert not any("v_mfma_f32_32x32x16_bf16" in l for l in found["k_run512_f16x3"])


def test_kernel_sources_have_one_code_path():
    """The kernel sources compile one way: the only macros a preprocessor conditional tests are the two phase timers (measurement builds with
    tools behind them: tools/prof_phases.sh, tools/prof_l512.py) and __HIPCC__ (common.hpp, shared with the host compiler).  Ablation arms,
    lost experiments and tunables behind `#ifndef X / #define X n` were removed once (profiles/ablation_arms_removed.txt); a new one fails
    here.  A tunable is a constexpr beside the comment with its measurement; an experiment that lost goes to tools/ubench/*.hip.txt."""
    allowed = {"DINER_HN_PROF", "DINER_L512_PROF", "__HIPCC__"}
    csrc = os.path.join(ROOT, "diner_amd", "csrc")
    found = {}
    for name in sorted(os.listdir(csrc)):
        with open(os.path.join(csrc, name)) as f:
            for no, line in enumerate(f, 1):
                m = re.match(r"\s*#\s*(if|ifdef|ifndef|elif)\b(.*)", line)
                if m:
                    tested = set(re.findall(r"[A-Za-z_]\w*", m.group(2).split("//")[0])) - {"defined"}
                    assert tested, f"{name}:{no}: conditional on a constant"
                    for macro in tested - allowed:
                        found.setdefault(macro, f"{name}:{no}")
    assert not found, f"compile-time switches in the kernel sources: {found}"


def test_env_switches_are_the_ones_the_tests_flip():
    """The library and its Python host read a fixed set of environment variables.  On the training path those are the seven seams
    tests/test_train_gpu.py flips to compare two routes inside one process (five read per call by the library, two by diner_amd/train.py);
    the A/B aids of rounds 3-6 were fixed at their defaults once (profiles/train_switches_removed.txt), their measurements stand in the
    comments beside the constexpr that replaced them.  A new getenv / os.environ read fails here: an experiment belongs in tools/ubench/
    (a stand-alone .hip, or .hip.txt once it has lost), a tunable is a constexpr beside its measurement."""
    csrc = os.path.join(ROOT, "diner_amd", "csrc")
    in_lib = {}
    for name in sorted(os.listdir(csrc)):
        with open(os.path.join(csrc, name)) as f:
            for no, line in enumerate(f, 1):
                calls = re.findall(r"\bgetenv\s*\(\s*([^)]*)\)", line)
                for arg in calls:
                    m = re.fullmatch(r'"(\w+)"\s*', arg)
                    assert m, f"{name}:{no}: getenv of something other than one string literal: {arg!r}"
                    in_lib.setdefault(m.group(1), f"{name}:{no}")
    hint = "; experiments go to tools/ubench/, tunables become a constexpr beside their measurement"
    want_lib = {"DINER_TRAIN_PROJ_TOUCHED", "DINER_TRAIN_PROJ_CAP", "DINER_TRAIN_LINZ_MAPSPACE", "DINER_TRAIN_SCATTER_SORTED", "DINER_TRAIN_VIEW_SHARED"}
    assert set(in_lib) == want_lib, f"getenv in the library: new {({k: in_lib[k] for k in set(in_lib) - want_lib})}, gone {sorted(want_lib - set(in_lib))}" + hint
    in_py = {}
    paths = [os.path.join(ROOT, "diner_amd", n) for n in sorted(os.listdir(os.path.join(ROOT, "diner_amd"))) if n.endswith(".py")]
    for d, _, names in sorted(os.walk(os.path.join(ROOT, "src"))):
        paths += [os.path.join(d, n) for n in sorted(names) if n.endswith(".py")]
    for path in paths:
        with open(path) as f:
            for no, line in enumerate(f, 1):
                if "environ" in line or "getenv" in line:
                    for var in re.findall(r"""["'](DINER_\w+)["']""", line):
                        in_py.setdefault(var, f"{os.path.relpath(path, ROOT)}:{no}")
    want_py = {"DINER_AMD_LIB", "DINER_AMD_MAX_POINTS", "DINER_AMD_PRECISION", "DINER_AMD_VIEW_GROUPS", "DINER_TRAIN_FUSED_FWD", "DINER_TRAIN_BATCH"}
    assert set(in_py) == want_py, f"os.environ in the Python host: new {({k: in_py[k] for k in set(in_py) - want_py})}, gone {sorted(want_py - set(in_py))}" + hint


def test_bench_line_contract():
    """The committed bench line (profiles/, produced by `python bench.py` on an MI355X) carries every field of the
    driver's contract, the roofline object and the CPU baseline object."""
    import json
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    import glob
    newest = sorted(glob.glob(os.path.join(root, "profiles", "r0*_bench_line_with_cpu_baseline.json")))[-1]
    with open(newest) as f:
        line = json.loads(f.read())
    with open(os.path.join(root, "BASELINE.json")) as f:
        base = json.load(f)
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert k in line, k
    assert line["metric"].split(" at ")[0] in base["metric"] and line["unit"] == "rays/s"
    assert line["higher_is_better"] is True and line["scaling"] == "strong" and line["vs_baseline"] is None
    assert line["data"] == "synthetic" and "workload" in line["config"] and "model" not in line["config"]
    # the headline line is the north_star configuration: one 800x600 frame of 480,000 rays per step, 128 samples per ray
    assert "north_star" in line["config"]["workload"] and line["config"]["frame"] == "800x600"
    assert line["config"]["rays_per_step"] == 480000 and line["config"]["samples_per_ray"] == 128
    assert "fp32" in line["modes"] and line["modes"]["fp32"]["rays_per_s"] > 0
    if "configs" in line:      # round 3: the other single-GPU BASELINE configs ride in the same line
        assert any("400x300" in k for k in line["configs"]) and sum("1024x1024" in k for k in line["configs"]) == 2
        assert "whole_path" in line["roofline"]
    if "frame_check" in line:      # round 4: the line says who took part and whether the sharded frame was checked; every modes / configs entry is a
        assert line["n_gpus"] == 1 and line["dist"] is None and line["backend"] is None      # median of >= 3 frames with its own roofline figures,
        assert "no collective" in line["config"]["parallelism"]                               # and the frame through the drop-in modules rides along
        for e in list(line["modes"].values()) + list(line["configs"].values()):
            assert e["steps"] >= 3 and len(e["ms_all"]) == e["steps"]
            rr = e["roofline"]
            assert abs(rr["frac"] - rr["achieved"] / rr["peak"]) < 1e-3 and 0 < rr["whole_path_frac"] < 1
        via = [v for k, v in line["configs"].items() if "through src.models" in k]
        assert len(via) == 1 and "4096 rays" in [k for k in line["configs"] if "through src.models" in k][0]
        assert abs(via[0]["vs_ops_level_headline"] - 1.0) < 0.03          # the module-level API costs < 3 % against the ops level
    r = line["roofline"]
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert k in r, k
    assert r["bound"] in ("hbm", "mfma") and r["unit"] in ("GB/s", "TFLOP/s")
    assert abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-3
    c = line["cpu_baseline"]
    for k in ("value", "unit", "cores", "kind", "sample"):
        assert k in c, k
    assert c["kind"] in ("reference", "port") and c["unit"] == "rays/s" and c["cores"] >= 1
    assert abs(line["value"] - line["config"]["rays_per_step"] / (line["ms_per_step"] * 1e-3)) < 0.01 * line["value"]
    # CPU baseline as SURVEY.md section 8d specifies it: >= 4096 rays, warm-up at size, >= 3 timed repeats, threads stated
    assert len(c["repeats_s"]) >= 3 and "4096 rays" in c["sample"] and c["host_threads"] >= c["cores"]
    if "train" in line:      # round 6: the line proves what it ran (VERDICT r5 #1a, #2)
        assert line["fallback_launches"] == 0, "the headline number is the exact-fp32 pass's, not the mode's it names"
        for e in list(line["modes"].values()) + list(line["configs"].values()):
            assert e["fallback_launches"] == 0
        en = line["energy"]
        assert set(("power_w", "sclk_mhz", "joule_per_mray", "power_samples")) <= set(en)
        if en["power_w"] is not None:
            assert 200 < en["power_w"] < 1500 and abs(en["joule_per_mray"] - en["power_w"] * line["ms_per_step"] * 1e-3 * line["steps"] /
                                                      (line["config"]["rays_per_step"] * line["steps"] / 1e6)) < 0.02 * en["joule_per_mray"]
        enc = line["encode"]
        assert enc["encode_ms"] > 0 and abs(enc["encode_ms"] - (enc["trunk_and_prep_ms"] + enc["relayout_ms"] + enc["hoist_ms"])) < 0.01
        t = line["train"]
        assert t["steps"] >= 5 and len(t["ms_all"]) == t["steps"] and t["batched"] is True
        assert t["config"]["objects"] == 4 and t["config"]["rays_per_object"] == 4096 and t["config"]["samples_per_ray"] == 40
        assert t["host_enqueue_ms"] <= 10.0, "the training step waits for the host again"
        assert abs(t["rays_per_s"] - 4 * 4096 / (t["ms_per_step"] * 1e-3)) < 0.01 * t["rays_per_s"]
        assert abs(t["frac"] - t["mfma_issued_tflops"] / 2500.0) < 1e-3 and 0 < t["frac"] < 1
        assert c["host_cores"] is None or c["host_cores"] <= c["host_threads"]


def test_png_writer_roundtrip(tmp_path):
    """diner_amd.imageio.write_png writes a valid 8-bit PNG (signature, chunk CRCs, zlib stream) that reads back bit-exact."""
    import numpy as np
    from diner_amd import imageio
    g = np.random.default_rng(0)
    for shape in ((37, 53, 3), (16, 16), (1, 1, 3)):
        a = g.integers(0, 256, size=shape, dtype=np.uint8)
        p = str(tmp_path / "x.png")
        imageio.write_png(p, a)
        assert np.array_equal(imageio.read_png(p), a)
