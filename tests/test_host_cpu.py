"""CPU tests of the product's host side: schedule scalars against the reference goldens, the C-ABI library
loads and exports every symbol include/esmdiff_hip.h declares (no compute without a GPU), loud failure
without a GPU."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from tests.recorded_math import recorded_math

ROOT = Path(__file__).resolve().parent.parent


@recorded_math
def test_schedule_matches_reference_goldens(golden_dir):
    from esmdiff_amd.schedule import CosineNoise, LogLinearNoise, ddpm_schedule, timestep_embedding
    g = np.load(golden_dir / "g1_schedules.npz")
    for T in (5, 25, 50):
        for nm, noise in (("loglinear", LogLinearNoise()), ("cosine", CosineNoise(1e-3))):
            s = ddpm_schedule(T, 1e-5, 1.0, noise)
            assert np.array_equal(s.timesteps.numpy(), g[f"timesteps_T{T}"])
            assert s.dt == float(g[f"dt_T{T}"])
            assert np.array_equal(s.sigma_t.numpy(), g[f"{nm}_sigma_t_T{T}"])
            assert np.array_equal(s.mc_t.numpy(), g[f"{nm}_mc_t_T{T}"])
            assert np.array_equal(s.mc_s.numpy(), g[f"{nm}_mc_s_T{T}"])
            assert s.t_freq.shape == (T + 1, 256)
    g2 = np.load(golden_dir / "g2_timestep.npz")
    sig = torch.from_numpy(g2["sigma"])
    assert np.array_equal(timestep_embedding(sig, 256).numpy(), g2["freq_embedding_256"])
    assert np.array_equal(timestep_embedding(sig, 7).numpy(), g2["freq_embedding_7"])


def test_library_exports_every_declared_symbol():
    from esmdiff_amd import _native
    from esmdiff_amd.build import build
    lib_path = build()
    assert lib_path.exists()
    surface = (ROOT / "include" / "esmdiff_hip.h").read_text()
    header = surface + (ROOT / "include" / "esmdiff_hip_test.h").read_text()
    header = re.sub(r"#ifdef ED_DEBUG.*?#endif /\* ED_DEBUG \*/", "", header, flags=re.S)   # the timing aid of debug builds
    assert "esmdiff_debug_graph_ab" not in header
    declared = set(re.findall(r"\b(esmdiff_[a-z0-9_]+)\s*\(", header))
    declared -= {"esmdiff_gemm_epilogue"}
    assert declared == set(_native.EXPORTS), declared ^ set(_native.EXPORTS)
    L = ctypes.CDLL(str(lib_path))
    for name in declared:
        assert hasattr(L, name), name
    # both operand-type builds of the kernels are linked in (csrc/ed_half.h: namespace ed = bf16, ed16 = f16)
    import subprocess
    syms = subprocess.run(["nm", "--defined-only", str(lib_path)], capture_output=True, text=True).stdout
    for fn in ("launch_gemm_bf16", "launch_attention", "launch_add_layernorm_bf16", "launch_qk_norm_rope", "launch_to_bf16"):
        assert f"_ZN2ed{len(fn)}{fn}" in syms and f"_ZN4ed16{len(fn)}{fn}" in syms, fn
    # ... but the DYNAMIC symbol table is the C ABI and nothing else: no C++ internal is exported
    dyn = subprocess.run(["nm", "-D", "--defined-only", str(lib_path)], capture_output=True, text=True).stdout
    exported = {ln.split()[-1] for ln in dyn.splitlines() if ln.strip()}
    assert not [n for n in exported if n.startswith("_Z")], sorted(n for n in exported if n.startswith("_Z"))[:5]
    assert exported == declared, exported ^ declared
    # the drop-in surface (esmdiff_hip.h) holds no per-kernel test entry point; those live in esmdiff_hip_test.h
    for name in ("esmdiff_gemm_bf16", "esmdiff_gemm_split", "esmdiff_split_rows", "esmdiff_layernorm_bf16", "esmdiff_attention_bf16",
                 "esmdiff_branch_linear_layernorm", "esmdiff_set_profiling", "esmdiff_attention_f16", "esmdiff_qk_norm_rope",
                 "esmdiff_add_layernorm", "esmdiff_geom_attention"):
        assert name not in re.findall(r"\b(esmdiff_[a-z0-9_]+)\s*\(", surface), name
    for name in ("esmdiff_ddpm_sample", "esmdiff_forward_logits", "esmdiff_ddpm_step", "esmdiff_gibbs_step", "esmdiff_engine_create",
                 "esmdiff_gibbs_step_rows", "esmdiff_ddpm_step_rows"):
        assert name in re.findall(r"\b(esmdiff_[a-z0-9_]+)\s*\(", surface), name
    # the product library carries no debug exports
    assert not hasattr(L, "esmdiff_debug_graph_ab") and not hasattr(L, "esmdiff_gemm_bf16_timed")
    assert L.esmdiff_abi_version() == 8


def test_config_dimensions():
    from esmdiff_amd.config import ESM3_OPEN, TINY
    assert ESM3_OPEN.ffn_hidden == 4096 and abs(ESM3_OPEN.residue_scale - 1.154700538) < 1e-7
    assert TINY.ffn_hidden == 1536 and TINY.d_model == TINY.n_heads * 64


def test_random_init_state_dict_layout():
    from esmdiff_amd.config import TINY
    from esmdiff_amd.weights import random_init_state_dict
    from oracle.esm3_ref import build_from_state_dict
    sd = random_init_state_dict(TINY, seed=0)
    assert sd["net.transformer.blocks.1.ffn.1.weight"].shape == (2 * 1536, 512)
    assert sd["net.output_heads.structure_head.3.weight"].shape == (4101, 512)
    assert sd["sigma_embedder.mlp.0.weight"].shape == (512, 256)
    net, emb = build_from_state_dict(TINY, sd)   # strict load into the oracle network
    x = torch.full((1, 6), 4096)
    seq = torch.tensor([[0, 5, 6, 7, 8, 2]])
    with torch.no_grad():
        out = net(structure_tokens=x, sequence_tokens=seq).structure_logits
    assert out.shape == (1, 6, 4101) and torch.isfinite(out).all()


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-GPU failure mode")
def test_no_silent_cpu_fallback():
    from esmdiff_amd.config import TINY
    from esmdiff_amd.engine import Engine, gemm_bf16
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        Engine(TINY, {}, 1, 8)
    with pytest.raises(RuntimeError):
        gemm_bf16(torch.zeros(2, 64, dtype=torch.bfloat16), torch.zeros(128, 64, dtype=torch.bfloat16), 0)


def test_product_library_reads_no_tuning_environment():
    """no ESMDIFF_* switch can change a dispatch path (and with it the last bits of the logits): r05 moved them
    behind -DED_DEBUG, r09 retired them; the product library's strings hold no ESMDIFF_* name except the C enum constants that appear in mangled
    template names / messages and ESMDIFF_DEBUG_SKIP, which it reads only to REFUSE to create an engine.  Callers choose the
    legitimate knobs through esmdiff_set_option, and esmdiff_get_build_info says which kind of build this is."""
    import re
    import subprocess
    from esmdiff_amd import _native as N
    out = subprocess.run(["strings", str(N.lib_path())], capture_output=True, text=True, check=True).stdout
    names = set(re.findall(r"ESMDIFF_[A-Z0-9_]+", out))
    enum_like = re.compile(r"ESMDIFF_(EPI|F32EPI|PRECISION|OPT|E|F32|BF16|OK|ABI|VOCAB|MASK|STRUCT)_?[A-Z0-9_]*$")
    stray = {n for n in names if not enum_like.match(n)} - {"ESMDIFF_DEBUG_SKIP", "ESMDIFF_"}
    assert not stray, f"the product library mentions environment switches: {sorted(stray)}"
    info = N.build_info()
    assert "abi=8" in info and "arch=gfx950" in info and "debug_env=0" in info, info
    for sym in ("esmdiff_set_option", "esmdiff_describe_plan", "esmdiff_get_build_info"):
        assert hasattr(N.lib(), sym)


def test_hand_placed_gemm_has_no_sgpr_reload_hazard():
    """tools/check_asm_hazards.py on the hand-placed GEMMs: csrc/gemm256w4.hip in both operand-type builds and
    csrc/gemm256w4_split.hip (compiled once).  hipcc may reload a spilled SGPR with v_readlane directly in front of an inline-asm
    LDS-DMA that uses it as scalar base — a VALU-writes-SGPR -> VMEM hazard (5 wait states) that nobody pads inside an asm
    statement; the first split-f16 build faulted that way at multi-tile launches (r04).  The check compiles to gfx950 assembly (no
    GPU needed) and must find no such pair; the split kernels, whose main loop has no slack at all, must not spill at all."""
    import subprocess
    import sys
    sys.path.insert(0, str(ROOT / "tools"))
    import check_asm_hazards as chk
    from esmdiff_amd.build import F16_FLAGS
    csrc = ROOT / "esmdiff_amd" / "csrc"
    for src, extra in ((csrc / "gemm256w4.hip", []), (csrc / "gemm256w4.hip", F16_FLAGS), (csrc / "gemm256w4_split.hip", [])):
        r = subprocess.run(["/opt/rocm/bin/hipcc", *chk.FLAGS, *extra, str(src), "-o", "/dev/stdout"], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        seen = 0
        for name, meta, hazards in chk.analyse(r.stdout):
            assert not hazards, (name, hazards[:3])
            seen += 1
            assert ("gemm256w4_split_kernel" in name) == (src.name == "gemm256w4_split.hip"), name
            if "gemm256w4_split_kernel" in name and "ELb0EEE" in name:   # gemm256w4_split_kernel<EPI, KSLICED = false>
                assert meta.get("vgpr_spill_count", 0) == 0, (name, meta)
                if "ILi4E" not in name:    # (the fused-SwiGLU epilogue keeps a few scalars in VGPR lanes; none is reloaded near asm)
                    assert meta.get("sgpr_spill_count", 0) == 0, (name, meta)
            assert meta.get("agpr_count") == 256, (name, meta)      # the 128 x 128 wave tile lives in the accumulation registers
        assert seen == 5, (src.name, extra, seen)   # 5 bf16 / f16 epilogues; 4 split epilogues + the K-sliced store kernel


def test_no_kernel_ships_the_packed_float_form_that_fails_beside_the_gemm():
    """r06 (profiles/r06_frames_two_queue_race.txt, third pass): v_pk_fma_f32 / v_pk_mul_f32 whose op_sel takes the LOW result half from
    the HIGH register of src1 (op_sel:[.,1,.]) compute that half without the product — fma returns C.lo, mul returns +-0 — in lanes
    48-63 whenever a wave of the product's 256x256 GEMM shares the SIMD (scratch/ubench/pk_opsel.hip: a 30-line self-checking kernel,
    every round).  hipcc's SLP vectoriser emits that form for 3x3 rotations; block 0's geometric kernel had it, ran beside the other
    queue's GEMM in the two-queue forward, and gave a few wrong (row, head) outputs per forward.  csrc/geom.hip is therefore compiled
    without SLP vectorisation (esmdiff_amd/build.py), and this check disassembles EVERY gfx950 code object inside the shipped
    library (no GPU needed): no kernel may hold the form, and the four geom_attention_kernel instantiations hold no packed float op."""
    import re
    import subprocess
    import tempfile
    from esmdiff_amd import _native as N
    llvm = Path("/opt/rocm/lib/llvm/bin")
    if not (llvm / "clang-offload-bundler").exists() or not (llvm / "llvm-objdump").exists():
        pytest.skip("no ROCm LLVM tools")
    with tempfile.TemporaryDirectory() as td:
        fat = Path(td) / "fat.bin"
        subprocess.run(["objcopy", "-O", "binary", "--only-section=.hip_fatbin", str(N.lib_path()), str(fat)], check=True)
        blob = fat.read_bytes()
        starts = [m.start() for m in re.finditer(b"__CLANG_OFFLOAD_BUNDLE__", blob)]
        assert starts, "no offload bundles in the library"
        geom_seen = kernels = packed_total = 0
        for n, i in enumerate(starts):
            j = starts[n + 1] if n + 1 < len(starts) else len(blob)
            bundle, co = Path(td) / f"b{n}.bundle", Path(td) / f"b{n}.co"
            bundle.write_bytes(blob[i:j])
            subprocess.run([str(llvm / "clang-offload-bundler"), "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                            f"--input={bundle}", f"--output={co}"], check=True, capture_output=True)
            text = subprocess.run([str(llvm / "llvm-objdump"), "-d", str(co)], capture_output=True, text=True, check=True).stdout
            for name, body in re.findall(r"^[0-9a-f]+ <([^>]+)>:\n(.*?)(?=^[0-9a-f]+ <|\Z)", text, re.S | re.M):
                kernels += 1
                for op, rest in re.findall(r"\b(v_pk_\w+|v_dot\w+)\b([^\n]*)", body):
                    packed_total += 1
                    sel = re.search(r"\bop_sel:\[([01,]+)\]", rest)
                    if sel:
                        bits = [int(b) for b in sel.group(1).split(",")]
                        # measured safe beside the GEMM with src1's HIGH register in the low half: v_pk_add_f32 (the LayerNorm kernels'
                        # horizontal add; 10 of 10 clean rounds where the fma / mul forms fail in every one).  Every other packed op
                        # with that op_sel is either known to fail (v_pk_fma_f32, v_pk_mul_f32) or untested: measure it with
                        # scratch/ubench/pk_opsel.hip before shipping it
                        measured_safe = ("v_pk_add_f32", "v_pk_fma_f16", "v_pk_mul_f16", "v_pk_add_f16")   # (the f16 forms swap halves of ONE register)
                        assert not (len(bits) > 1 and bits[1]) or op in measured_safe, (name, op + rest.split("//")[0].rstrip())
                if "geom_attention_kernel" in name:
                    packed = re.findall(r"\bv_pk_\w+", body)
                    assert not packed, (name, sorted(set(packed)))
                    geom_seen += 1
        assert geom_seen == 4, geom_seen
        assert kernels > 200 and packed_total > 1000, (kernels, packed_total)     # the scan saw the library (and its packed ops)
