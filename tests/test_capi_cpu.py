"""CPU-side checks of the product library: it builds, loads, exports every symbol the
public header declares, and refuses to compute without a GPU (no CPU fallback)."""
import os
import re
import subprocess
import sys

import pytest

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "sketchlib_dist.h")


def _declared_in_header():
    text = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(skl_[a-z0-9_]+)\s*\(", text)))


def test_header_symbols_all_exported(skl):
    import sketchlib.rust_amd as pkg

    declared = _declared_in_header()
    assert len(declared) >= 20
    out = subprocess.check_output(["nm", "-D", "--defined-only", pkg.library_path()], text=True)
    exported = set(re.findall(r" T (skl_[a-z0-9_]+)", out))
    missing = [s for s in declared if s not in exported]
    assert not missing, f"declared in the header but not exported: {missing}"
    # and the ctypes binding covers the same set
    assert sorted(skl.DECLARED_SYMBOLS) == declared


def test_nothing_but_the_header_and_the_kernels_is_exported():
    """The strong symbols of the dynamic table: the functions of the public header, the kernels and their launchers in namespace
    skl:: (scripts/microbench/kslice_trace links against them), and nothing else of the host layer -- what the translation
    units share among themselves is declared SKL_INTERNAL in capi_internal.hpp and stays hidden."""
    import sketchlib.rust_amd as pkg

    pkg.build_library()
    declared = set(_declared_in_header())
    toolchain = re.compile(r"__hip_cuid_[0-9a-f]+")          # one byte per HIP translation unit, emitted by hipcc: the only such symbols seen
    for lib in (pkg.library_path(), pkg.build_ab_library()):
        out = subprocess.check_output(["nm", "-D", "--defined-only", lib], text=True)
        strong = [l.split() for l in out.splitlines() if len(l.split()) == 3 and l.split()[1] in "TDBRGS"]
        text = {name for _a, kind, name in strong if kind == "T" and not name.startswith("_ZN3skl")}
        assert text == declared, (lib, sorted(text ^ declared))
        data = [name for _a, kind, name in strong if kind != "T" and not name.startswith("_ZN3skl") and not toolchain.fullmatch(name)]
        assert not data, (lib, data)
        assert "free_plans" not in out and "next_generation" not in out


def test_product_library_has_no_ab_kernels_or_switches():
    """The forms kept for A/B timing (the round-2/3 forms of the chunk-split kernel's tile shapes) and the
    timing-only ablations, whose outputs are wrong by construction, exist only in the -DSKL_AB build; the
    product library has neither the instantiations nor the environment switches.  (The kernels that lost
    their A/Bs in rounds 1-3 are not built at all: experiments/dropped_kernels/.)"""
    import sketchlib.rust_amd as pkg

    pkg.build_library()
    syms = subprocess.check_output(["nm", "-D", "--defined-only", pkg.library_path()], text=True)
    demangled = subprocess.check_output(["c++filt"], input=syms, text=True)
    kernels = sorted(set(re.findall(r"skl::(pair_kernel\w*<[^>]*>)", demangled)))
    assert kernels, "no pair kernel exported?"
    for k in kernels:
        # chunk-split kernel: 16 x 128 and 32 x 128 tiles in the packed-count form only (32 x 128: blocks of 2 rows, held to
        # 4 waves per SIMD), ablation parameter 0; ksplit fallback: 8-row tiles
        # (last three parameters: the segmented walk of sketches beyond 65 535 bins, k-sliced forms only; tile pruning, the
        # single-k 32 x 128 form of the symmetric self kNN only; the fused core/accessory epilogue, which lost its A/B
        # (profiles/r05_fused_epilogue.md) and exists in the A/B build only)
        assert re.fullmatch(r"pair_kernel_kslice<16, 2, [01], true, 0, true, 4, 0, (true|false), false, false>|"
                            r"pair_kernel_kslice<16, 2, [012], false, 0, true, 1, 0, false, false, false>|"
                            r"pair_kernel_kslice<32, 2, [01], true, 0, true, 2, 4, (true|false), false, false>|"
                            r"pair_kernel_kslice<32, 2, 1, true, 0, true, 2, 4, false, true, false>|"
                            r"pair_kernel_kslice<32, 2, [012], false, 0, true, 2, 4, false, false, false>|pair_kernel_ksplit<8, [012], 8, false>", k), k
    blob = open(pkg.library_path(), "rb").read()
    for needle in (b"SKL_KNN_SYMMETRIC", b"SKL_TOPK_STREAM", b"SKL_KNN_ROW_FLAGS", b"SKL_CAND_KERNEL", b"SKL_CAND_ROW_ORDER", b"SKL_CAND_SYMMETRIC",
                   b"SKL_REFHEAP_WAVE", b"SKL_ROUND_PRIORITY", b"SKL_MID_BAND", b"SKL_K_SLICES", b"SKL_KNN_PRUNE", b"SKL_KNN_SPARSE", b"SKL_KNN_PANEL", b"SKL_EARLY_BREAK", b"SKL_HALF_TILES",
                   b"SKL_INLINE_PREFIX", b"SKL_KNN_OVERLAP", b"SKL_SKETCH_KERNEL", b"pair_cand_kernel",
                   b"SKL_FUSE_EPILOGUE", b"SKL_FUSE_VARIANT", b"pair_kernel_lds", b"SKL_KSLICE_ABLATE", b"SKL_LDS_ABLATE", b"SKL_KERNEL", b"SKL_KSLICE_SHAPE",
                   b"SKL_LDS_SHAPE", b"SKL_FORCE_NA", b"SKL_PAIR_VARIANT", b"SKL_PERSIST"):
        assert needle not in blob, needle
    # and no getenv on the launch path: the environment is read in capi_knobs.cpp and nowhere else -- not in another
    # translation unit of the C ABI, not in a kernel file, not in the switches' table or a plan header -- by read_knobs(), once per context
    csrc = os.path.join(ROOT, "sketchlib.rust_amd", "csrc")
    capi = sorted(f for f in os.listdir(csrc) if f.startswith("capi") and f.endswith(".cpp"))
    assert "capi.cpp" not in capi and {"capi_ctx.cpp", "capi_knobs.cpp", "capi_tables.cpp", "capi_sketches.cpp", "capi_eb.cpp", "capi_dense.cpp"} <= set(capi)
    plans = sorted(f for f in os.listdir(csrc) if f.endswith("_plan.hpp")) + ["work_map.hpp", "eb_stripes.hpp", "knobs.hpp", "knobs.def", "dist_tables.hpp", "capi_internal.hpp"]
    assert len(plans) >= 12
    src = {f: open(os.path.join(csrc, f)).read() for f in capi + plans + sorted(f for f in os.listdir(csrc) if f.endswith(".hip"))}
    assert len(src) >= 40
    assert src["capi_knobs.cpp"].count("getenv(") == 1
    for f, text in src.items():
        if f != "capi_knobs.cpp":
            assert "getenv" not in text and "env_int(" not in text, f
    # read_knobs(): its definition, skl_ctx_create, skl_ctx_reload_env, the A/B build's refresh at every API entry
    calls = {f: text.count("read_knobs(") for f, text in src.items() if f.endswith(".cpp") and "read_knobs(" in text}
    assert calls == {"capi_knobs.cpp": 1, "capi_ctx.cpp": 3}, calls
    ctx = src["capi_ctx.cpp"]
    for fn in ("int ctx_bind(skl_ctx *ctx)", 'extern "C" int skl_ctx_create(', 'extern "C" int skl_ctx_reload_env('):
        body = ctx[ctx.index(fn):]
        assert "ctx->knobs = read_knobs();" in body[:body.index("\n}\n")], fn
    # ... and the reader behind it (knobs.hpp knobs_from) is reached from capi_knobs.cpp alone: read_knobs() and the A/B build's
    # once-per-process SKL_FORCE_LOG_VARIANT inside the cached probe of the host's logarithm
    uses = {f: text.count("knobs_from(") for f, text in src.items() if f.endswith((".cpp", ".hip")) and "knobs_from(" in text}
    assert uses == {"capi_knobs.cpp": 2}, uses
    assert sum(text.count("ab_forced_log_variant()") for f, text in src.items() if f.endswith(".cpp")) == 2
    assert src["capi_tables.cpp"].count("ab_forced_log_variant()") == 1 and "static const int variant = [] {" in src["capi_tables.cpp"]


def test_library_has_gfx950_code_object():
    import sketchlib.rust_amd as pkg

    pkg.build_library()
    blob = open(pkg.library_path(), "rb").read()
    assert b"gfx950" in blob, "no gfx950 code object embedded"
    assert b"pair_kernel" in blob


def test_no_cpu_fallback(skl):
    if skl.device_count() > 0:
        pytest.skip("a GPU is present; the refusal path is only reachable without one")
    with pytest.raises(skl.SklError) as e:
        skl.Context(0)
    assert e.value.code == skl.ERR_NO_DEVICE
    assert "no CPU path" in e.value.message
    import numpy as np

    p = skl.params()
    with pytest.raises(skl.SklError) as e:
        skl.self_dists_all_host(np.zeros(2 * 2 * 14, dtype=np.uint64), 2, [17, 21], 1, p)
    assert e.value.code == skl.ERR_NO_DEVICE


def test_product_never_imports_oracle():
    """The oracle is test infrastructure: nothing under the package or include/ may
    reference it."""
    pkg_dir = os.path.join(ROOT, "sketchlib.rust_amd")
    offenders = []
    for root, _d, files in os.walk(pkg_dir):
        if "_build" in root or "__pycache__" in root:
            continue
        for f in files:
            if f.endswith((".py", ".cpp", ".hip", ".h", ".hpp", "Makefile")):
                text = open(os.path.join(root, f), errors="replace").read()
                if re.search(r"(from|import)\s+oracle|oracle/|sketchlib_oracle|sko_", text):
                    offenders.append(os.path.join(root, f))
    assert not offenders, offenders


def test_unmatched_host_log_is_reported_through_ctx_flags():
    """skl_log_variant() == -1 (this host's libm log() is neither form the device restates) must reach the
    caller: skl_ctx_flags() carries SKL_CTX_FLAG_LOG_UNMATCHED and the library prints nothing itself.  The
    branch is forced through the A/B build's SKL_FORCE_LOG_VARIANT (the probe is cached per process, so each
    case runs in its own)."""
    import sketchlib.rust_amd as pkg

    lib = pkg.build_ab_library()
    code = ("import ctypes, sys; L = ctypes.CDLL(sys.argv[1]); L.skl_ctx_flags.restype = ctypes.c_uint; "
            "L.skl_ctx_flags.argtypes = [ctypes.c_void_p]; print(L.skl_log_variant(), L.skl_ctx_flags(None))")
    for forced, want in (("-1", "-1 1"), ("0", "0 0"), ("1", "1 0"), (None, None)):
        env = dict(os.environ)
        env.pop("SKL_FORCE_LOG_VARIANT", None)
        if forced is not None:
            env["SKL_FORCE_LOG_VARIANT"] = forced
        res = subprocess.run([sys.executable, "-c", code, lib], env=env, capture_output=True, text=True, timeout=120)
        assert res.returncode == 0, res.stderr
        assert res.stderr.strip() == "", "the library itself prints nothing: " + res.stderr
        if want is not None:
            assert res.stdout.split() == want.split(), (forced, res.stdout)
        else:       # unforced: this image's glibc 2.35 matches one of the two forms
            v, f = res.stdout.split()
            assert v in ("0", "1") and f == "0"
    # the product library has no such switch
    assert b"SKL_FORCE_LOG_VARIANT" not in open(pkg.library_path(), "rb").read()
    # and the CLI warns once when a completeness correction meets the flag.  The form checked: ONE shared helper, defined
    # once (host/cli/common.cpp: the flag test and the warning), called from exactly the two command files whose commands
    # take a completeness correction -- dist.cpp (`dist`) and inverted.cpp (`inverted precluster`), once each, under the
    # condition that a completeness file was given -- and the flag and the warning text are used nowhere else.
    cli_dir = os.path.join(ROOT, "sketchlib.rust_amd", "csrc", "host", "cli")
    cli = {f: open(os.path.join(cli_dir, f)).read() for f in sorted(os.listdir(cli_dir))}
    assert cli["common.cpp"].count("if (skl_ctx_flags(ctx) & SKL_CTX_FLAG_LOG_UNMATCHED) log.warn(LOG_UNMATCHED_WARNING);") == 1
    assert {f: s.count("SKL_CTX_FLAG_LOG_UNMATCHED") for f, s in cli.items() if "SKL_CTX_FLAG_LOG_UNMATCHED" in s} == \
        {"common.cpp": 1, "common.hpp": 1}            # (the header: a comment)
    assert {f: s.count("log.warn(LOG_UNMATCHED_WARNING)") for f, s in cli.items() if "log.warn(LOG_UNMATCHED_WARNING)" in s} == {"common.cpp": 1}
    calls = {f: s.count("warn_if_log_unmatched(") for f, s in cli.items() if "warn_if_log_unmatched(" in s}
    assert calls == {"common.hpp": 1, "common.cpp": 1, "dist.cpp": 1, "inverted.cpp": 1}, calls
    assert "if (ref_comp || query_comp) warn_if_log_unmatched(log, dev[0].ctx());" in cli["dist.cpp"]
    assert "if (comp) warn_if_log_unmatched(log, dev.ctx());" in cli["inverted.cpp"]
    precluster = cli["inverted.cpp"].split("int run_inverted_precluster(")[1]
    assert "warn_if_log_unmatched(" in precluster


def _kernel_metadata(lib_path):
    """{demangled kernel name: (vgprs, scratch bytes per lane, LDS bytes)} from the gfx950 code object in the library."""
    import tempfile

    llvm = "/opt/rocm/lib/llvm/bin"
    notes = ""
    with tempfile.TemporaryDirectory() as tmp:
        fat = os.path.join(tmp, "fat.bin")
        subprocess.check_call(["objcopy", "-O", "binary", "--only-section=.hip_fatbin", lib_path, fat])
        blob = open(fat, "rb").read()
        magic = b"__CLANG_OFFLOAD_BUNDLE__"          # one bundle per object file linked into the library
        starts = [m.start() for m in re.finditer(re.escape(magic), blob)]
        for n, a in enumerate(starts):
            piece, dev = os.path.join(tmp, f"bundle{n}.bin"), os.path.join(tmp, f"dev{n}.o")
            open(piece, "wb").write(blob[a:starts[n + 1] if n + 1 < len(starts) else len(blob)])
            subprocess.check_call([f"{llvm}/clang-offload-bundler", "--unbundle", "--type=o", f"--input={piece}",
                                   "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--output={dev}"])
            notes += subprocess.check_output([f"{llvm}/llvm-readelf", "--notes", dev], text=True)
    out = {}
    for blk in notes.split("- .agpr_count:")[1:]:
        def field(name):
            return re.search(r"\." + name + r":\s+(\S+)", blk).group(1)
        name = subprocess.check_output(["c++filt", field("name")], text=True).strip()
        out[name] = (int(field("vgpr_count")), int(field("private_segment_fixed_size")), int(field("group_segment_fixed_size")))
    return out


def test_register_budget_of_the_shipped_pair_kernels():
    """The pair kernels are built for a fixed occupancy, and hipcc's register allocation of them has proved fragile
    (one more run-time condition on the half-tile flags spilled 11 registers of the 16-row k-sliced form; wrapping the
    tile walk in a lambda spilled the 32-row one; 64-bit per-lane DMA pointers made the 4-wave all-k form reload
    registers at every stage).  What ships: EVERY form holds 4 waves per SIMD (<= 128 VGPRs, <= 40 KB of LDS) -- the
    16-row k-sliced ones without a byte of scratch, the 32-row ones with a handful of values spilled OUTSIDE their stage
    loops -- and the all-k forms keep their per-k totals (<= 192 B per lane) in private memory by design."""
    import sketchlib.rust_amd as pkg

    pkg.build_library()
    meta = {k: v for k, v in _kernel_metadata(pkg.library_path()).items() if "pair_kernel_kslice" in k}
    assert len(meta) == 15, sorted(meta)
    for name, (vgpr, scratch, lds) in meta.items():
        r, _jl, _mode, ksl = re.search(r"pair_kernel_kslice<(\d+), (\d+), (\d+), (true|false)", name).groups()
        big, prune, fuse = re.search(r", (true|false), (true|false), (true|false)>\(", name).groups()
        assert fuse == "false", name
        if prune == "true":
            # tile pruning (the single-k 32 x 128 form): + 544 B of LDS for the column bounds and the votes, a handful of values
            # spilled, one reload of them inside the walk
            assert vgpr <= 128 and lds <= 40 * 1024 and scratch <= 64, (name, vgpr, scratch, lds)
        elif big == "true":
            # the segmented walk (sketches beyond 65 535 bins): 32-bit totals in private memory, touched once per 1 016 chunks
            assert vgpr <= 128 and lds <= 40 * 1024 and scratch <= 448, (name, vgpr, scratch, lds)
        elif ksl == "true":
            assert vgpr <= 128 and lds <= 40 * 1024, (name, vgpr, lds)
            assert scratch == 0 if r == "16" else scratch <= 32, (name, scratch)
        else:
            assert vgpr <= 128 and lds <= 40 * 1024, (name, vgpr, lds)
            assert scratch <= 256, (name, scratch)


def test_register_budget_of_the_candidate_list_and_replay_kernels():
    """pair_cand_rows_kernel<TRIPS> keeps the row's planes in registers (7 x 8 bytes per lane and trip): every form must do
    so without scratch and stay at 4 waves per SIMD or better (<= 128 VGPRs; one or two trips <= 64: 8 waves); the
    one-wave-per-row heap replays take <= 20 KB of LDS per workgroup of 4 rows, so that 8 workgroups fit a CU."""
    import sketchlib.rust_amd as pkg

    pkg.build_library()
    meta = _kernel_metadata(pkg.library_path())
    rows = {k: v for k, v in meta.items() if "pair_cand_rows_kernel" in k}
    assert len(rows) == 6, sorted(rows)
    for name, (vgpr, scratch, lds) in rows.items():
        trips = int(re.search(r"pair_cand_rows_kernel<(\d+)>", name).group(1))
        assert scratch == 0 and lds == 0, (name, scratch, lds)
        assert vgpr <= (64 if trips <= 2 else 128), (name, vgpr)
    for kernel in ("topk_refheap_wave_kernel", "refheap_merge_wave_kernel"):
        (vgpr, scratch, lds), = [v for k, v in meta.items() if kernel in k]
        assert scratch == 0 and vgpr <= 64 and lds <= 20 * 1024, (kernel, vgpr, scratch, lds)


def test_register_budget_of_the_early_break_epilogues():
    """The lean early-break epilogue (epilogue.hip coreacc_epilogue_lean_kernel<SLICED, NK>) is bound by the instructions it
    issues and hides its loads behind other waves: the six forms without a completeness correction must stay at 8 waves per SIMD (<= 64 VGPRs) without scratch, the six with one at 5;
    the general kernel at 5 (<= 96; with a completeness correction 4: <= 128), the kNN bands' at 4 or better."""
    import sketchlib.rust_amd as pkg

    pkg.build_library()
    meta = _kernel_metadata(pkg.library_path())
    lean = {k: v for k, v in meta.items() if "coreacc_epilogue_lean_kernel" in k}
    assert len(lean) == 12, sorted(lean)
    for name, (vgpr, scratch, lds) in lean.items():
        if name.rstrip().endswith("true>(skl::EpilogueArgs)"):   # <SLICED, NK, COMP = true>: calls the restated logarithm out of line
            assert scratch <= 64 and vgpr <= 96, (name, vgpr, scratch)
        else:
            assert scratch == 0 and vgpr <= 64, (name, vgpr, scratch)
    for name, (vgpr, scratch, lds) in meta.items():
        if "coreacc_epilogue_kernel_r6<false>" in name:
            assert scratch == 0 and vgpr <= 96, (name, vgpr, scratch)
        if "coreacc_epilogue_kernel_r6<true>" in name or "coreacc_epilogue_knn_kernel" in name:
            assert scratch == 0 and vgpr <= 128, (name, vgpr, scratch)
