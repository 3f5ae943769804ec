"""The C-ABI library loads and exports every symbol include/nerfsig.h declares (no compute calls: no GPU here)."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    text = open(os.path.join(ROOT, "include", "nerfsig.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"^(?:int|size_t|const char \*|void \*)\s*(\w+)\s*\(", text, flags=re.M)))


@pytest.fixture(scope="module")
def native():
    from nerf_signature_amd import build, _native
    build.build()
    return _native


def test_header_and_loader_agree(native):
    assert _declared() == sorted(native.SIGNATURES)


def test_every_declared_symbol_is_exported(native):
    assert native.verify_exports() == _declared()
    assert native.fn("nsig_abi_version")() == 1


def test_host_only_queries(native):
    assert native.fn("rm_march_train_scratch_bytes")(4096, 1024) == 4096 * 1024 * 4
    assert native.fn("mlp_packed_bytes")() == 3 * (24 + 24) * 64 * 16          # split-bf16 hi + lo and fp16 fragments, forward + backward
    before = native.fn("mlp_get_precision")()
    assert before in (0, 1)
    native.set_mlp_precision("bf16x3")
    assert native.fn("mlp_get_precision")() == 0 and "split-bf16" in native.mlp_precision_name() and native.mlp_mfma_per_wave() == (72, "bf16")
    native.set_mlp_precision("f16")
    assert native.fn("mlp_get_precision")() == 1 and native.mlp_mfma_per_wave() == (24, "f16")
    with pytest.raises(ValueError):
        native.call("mlp_set_precision", 7)
    native.call("mlp_set_precision", before)


def test_decoder_workspace_layout_is_host_only(native):
    """dec_workspace_layout: 72 offsets in carve order, increasing, 256-byte aligned, the last below dec_workspace_bytes; an unsupported shape and a null
    pointer are refused."""
    c = native._c
    for shape in ((32, 3, 12, 12), (2, 3, 32, 32), (3, 3, 1, 1), (2, 25, 6, 6)):
        off, geom = (c.c_uint64 * 72)(), (c.c_uint32 * 6)()
        native.call("dec_workspace_layout", *shape, off, geom)
        off, total = list(off), native.fn("dec_workspace_bytes")(*shape)
        assert off[0] == 0 and all(b > a for a, b in zip(off, off[1:])) and all(o % 256 == 0 for o in off) and off[-1] + 4 * shape[0] <= total
        B, _, H, W = shape
        ntile, npair, rows_max, nband, R, RS = geom
        assert ntile == -(-H * W // 32) and npair == -(-ntile // 2) and nband == -(-H // R) and RS % 8 == 0 and RS >= W + 2 and 3 <= rows_max <= H + 2
        assert off[1] - off[0] == -(-B * H * W * 64 * 4 // 256) * 256                 # x_0 is [B][P][64] fp32
    with pytest.raises(ValueError, match="unsupported image shape 193x3x5x5"):
        native.call("dec_workspace_layout", 193, 3, 5, 5, (c.c_uint64 * 72)(), (c.c_uint32 * 6)())
    with pytest.raises(ValueError, match="unsupported image shape"):
        native.call("dec_workspace_layout", 2, 33, 6, 6, (c.c_uint64 * 72)(), (c.c_uint32 * 6)())
    with pytest.raises(ValueError, match="null pointer"):
        native.call("dec_workspace_layout", 2, 3, 6, 6, None, (c.c_uint32 * 6)())
    assert native.SIGNATURES["dec_workspace_layout"] == [c.c_uint32] * 4 + [native._vp, native._vp]


def test_argument_validation_needs_no_gpu(native):
    with pytest.raises(ValueError, match="null pointer"):
        native.call("rm_morton3D", None, 4, None, None)
    with pytest.raises(ValueError, match="out of range"):
        native.call("hg_codebook_presum", (native._vp * 1)(), 0, native._vp(16), None)
    # field_bwd_wgrad (the fused stage-1 backward): null pointers and its point range (32-bit lane byte offsets) are refused before anything is launched
    d = native._vp(256)
    with pytest.raises(ValueError, match="null pointer"):
        native.call("field_bwd_wgrad", 64, None, None, d, d, d, d, d, d, d, d, d, d, d, d, d, d, None)
    with pytest.raises(ValueError, match="out of range"):
        native.call("field_bwd_wgrad", (1 << 26) + 1, None, d, d, d, d, d, d, d, d, d, d, d, d, d, d, d, None)
    with pytest.raises(ValueError, match="16-byte aligned"):
        native.call("field_bwd_wgrad", 64, None, d, d, d, d, d, d, native._vp(264), d, d, d, d, d, d, d, d, None)
    # the slice owners store rows as 16-byte vectors: every gradient table of hg_levels_scatter has to be aligned
    tables = (native._vp * 16)(*([256] * 15 + [264]))
    with pytest.raises(ValueError, match="gradient table 15 must be 16-byte aligned"):
        native.call("hg_levels_scatter", d, 64, None, 1.0, d, 64, d, tables, None)
    # ... and the form with the optimiser step inside the owners refuses a misaligned moment table before it touches a step count
    good, bad = (native._vp * 16)(*([256] * 16)), (native._vp * 16)(*([256] * 3 + [264] + [256] * 12))
    with pytest.raises(ValueError, match="table 3 must be 16-byte aligned"):
        native.call("hg_levels_scatter_adam", d, 64, None, 1.0, d, 64, d, good, bad, good, good, d, 0.9, 0.99, 1e-15, 1.0, d, None)
    with pytest.raises(ValueError, match="null pointer"):
        native.call("hg_levels_scatter_adam", d, 64, None, 1.0, d, 64, d, good, good, good, good, None, 0.9, 0.99, 1e-15, 1.0, d, None)
    assert native.fn("field_bwd_wgrad_scratch_bytes")(1) == 12 * 1024 * 4 and native.fn("field_bwd_wgrad_scratch_bytes")(10 ** 6) == 256 * 12 * 1024 * 4


def test_optimiser_and_codebook_refusals_word_for_word(native):
    """Every refusal of the opt_* entry points and of hg_codebook_presum / hg_codebook_presum_sel / hg_fanout_grad that comes before any launch, by its whole message:
    null list, D / n out of range, a null or a misaligned element, misaligned G / S / S_next, opt_ema_update's tensor count and decay range."""
    vp, fl, u32 = native._vp, native._fl, native._u32
    d, off = vp(256), vp(264)                                # an aligned and a misaligned address (nothing is dereferenced on the device side of a refusal)
    arr = lambda *a: (vp * len(a))(*a)
    ok2, ok4 = arr(256, 512), arr(256, 512, 768, 1024)
    hp = (0.9, 0.99, 1e-15)

    def refused(name, message, *args):
        with pytest.raises(ValueError) as e:
            native.call(name, *args)
        assert str(e.value) == f"{name} failed (code 1): {name}: {message}"

    # opt_codebook_adam(G, params, exp_avg, exp_avg_sq, D, beta1, beta2, eps, step_sizes, inv_bc2, grad_scale, stream)
    ss = (fl * 4)(1, 1, 1, 1)
    adam = lambda G=d, p=ok2, m=ok2, v=ok2, D=2, s=ss: ("opt_codebook_adam", G, p, m, v, D, *hp, s, ss, 1.0, None)
    for a, msg in ((adam(p=None), "null pointer"), (adam(G=None), "null pointer"), (adam(s=None), "null pointer"), (adam(D=0), "D=0 out of range"), (adam(D=65), "D=65 out of range"),
                   (adam(G=off), "G must be 16-byte aligned"), (adam(m=arr(256, None)), "table 1 has a null pointer"), (adam(v=arr(264, 256)), "table 0 is not 16-byte aligned")):
        refused(a[0], msg, *a[1:])

    # opt_codebook_adam_sel(G, params, exp_avg, exp_avg_sq, steps, message, D, lr, beta1, beta2, eps, grad_scale, scratch, stream) and its _next form (+ next_message, S_next)
    for name, tail in (("opt_codebook_adam_sel", ()), ("opt_codebook_adam_sel_next", (d, d))):
        sel = lambda G=d, p=ok4, m=ok4, v=ok4, st=ok4, msg=d, D=2, lr=d, sc=d: (G, p, m, v, st, msg, D, lr, *hp, 1.0, sc, *tail, None)
        refused(name, "null pointer", *sel(st=None))
        refused(name, "null pointer", *sel(msg=None))
        refused(name, "null pointer", *sel(sc=None))
        refused(name, "D=0 out of range", *sel(D=0))
        refused(name, "D=65 out of range", *sel(D=65))
        refused(name, "G must be 16-byte aligned", *sel(G=off))
        refused(name, "table 2 has a null pointer", *sel(st=arr(256, 512, None, 1024)))
        refused(name, "table 3 has a null pointer", *sel(p=arr(256, 512, 768, None)))
        refused(name, "table 1 is not 16-byte aligned", *sel(m=arr(256, 520, 768, 1024)))
    nxt = lambda nm, S: (d, ok4, ok4, ok4, ok4, d, 2, d, *hp, 1.0, d, nm, S, None)
    for nm, S in ((None, d), (d, None), (d, off)):
        refused("opt_codebook_adam_sel_next", "next_message / S_next null or S_next not 16-byte aligned", *nxt(nm, S))

    # the dense entry points launch group by group: a null element at index 0 is refused before the first launch
    one, none1, n1, n0 = arr(256), arr(None), (u32 * 1)(8), (u32 * 1)(0)
    host = lambda p=one, g=one, m=one, v=one, numel=n1, s=ss: ("opt_adam_dense_host", 1, p, g, m, v, numel, s, ss, *hp, 1.0, None)
    dense = lambda p=one, g=one, m=one, v=one, st=one, numel=n1, lr=d, sc=d: ("opt_adam_dense", 1, p, g, m, v, st, numel, lr, *hp, 1.0, sc, None)
    for a, msg in ((host(p=None), "null pointer"), (host(numel=None), "null pointer"), (host(s=None), "null pointer"), (host(g=none1), "tensor 0 has a null pointer or no elements"),
                   (host(v=none1), "tensor 0 has a null pointer or no elements"), (host(numel=n0), "tensor 0 has a null pointer or no elements"),
                   (dense(m=None), "null pointer"), (dense(st=None), "null pointer"), (dense(lr=None), "null pointer"), (dense(sc=None), "null pointer"),
                   (dense(p=none1), "tensor 0 has a null pointer or no elements"), (dense(st=none1), "tensor 0 has a null pointer or no elements"),
                   (dense(numel=n0), "tensor 0 has a null pointer or no elements")):
        refused(a[0], msg, *a[1:])

    # opt_ema_update(n, params, shadow, numel, num_updates, decay, stream): one launch behind every check
    n2 = (u32 * 2)(8, 8)
    ema = lambda n=2, p=ok2, s=ok2, numel=n2, nu=d, decay=0.95: ("opt_ema_update", n, p, s, numel, nu, decay, None)
    for a, msg in ((ema(p=None), "null pointer"), (ema(nu=None), "null pointer"), (ema(n=0), "1 .. 32 tensors, decay in [0, 1]"), (ema(n=33), "1 .. 32 tensors, decay in [0, 1]"),
                   (ema(decay=-0.01), "1 .. 32 tensors, decay in [0, 1]"), (ema(decay=1.01), "1 .. 32 tensors, decay in [0, 1]"),
                   (ema(s=arr(256, None)), "tensor 1 has a null pointer or no elements"), (ema(p=arr(None, 256)), "tensor 0 has a null pointer or no elements"),
                   (ema(numel=(u32 * 2)(8, 0)), "tensor 1 has a null pointer or no elements")):
        refused(a[0], msg, *a[1:])

    # hg_codebook_presum(tables, D, S, stream), hg_codebook_presum_sel(all_tables, message, D, S, stream), hg_fanout_grad(G, grads, D, accumulate, stream)
    refused("hg_codebook_presum", "null pointer", None, 2, d, None)
    refused("hg_codebook_presum", "null pointer", ok2, 2, None, None)
    refused("hg_codebook_presum", "D=0 out of range [1,64]", ok2, 0, d, None)
    refused("hg_codebook_presum", "D=65 out of range [1,64]", ok2, 65, d, None)
    refused("hg_codebook_presum", "table 1 is null or not 16-byte aligned", arr(256, None), 2, d, None)
    refused("hg_codebook_presum", "table 0 is null or not 16-byte aligned", arr(264, 256), 2, d, None)
    refused("hg_codebook_presum", "S must be 16-byte aligned", ok2, 2, off, None)
    refused("hg_codebook_presum_sel", "null pointer", None, d, 2, d, None)
    refused("hg_codebook_presum_sel", "null pointer", ok4, None, 2, d, None)
    refused("hg_codebook_presum_sel", "D=0 out of range [1,64]", ok4, d, 0, d, None)
    refused("hg_codebook_presum_sel", "D=65 out of range [1,64]", ok4, d, 65, d, None)
    refused("hg_codebook_presum_sel", "table 3 is null or not 16-byte aligned", arr(256, 512, 768, None), d, 2, d, None)
    refused("hg_codebook_presum_sel", "table 2 is null or not 16-byte aligned", arr(256, 512, 776, 1024), d, 2, d, None)
    refused("hg_codebook_presum_sel", "S must be 16-byte aligned", ok4, d, 2, off, None)
    refused("hg_fanout_grad", "null pointer", None, ok2, 2, 0, None)
    refused("hg_fanout_grad", "null pointer", d, None, 2, 0, None)
    refused("hg_fanout_grad", "D=0 out of range", d, ok2, 0, 0, None)
    refused("hg_fanout_grad", "D=65 out of range", d, ok2, 65, 1, None)
    refused("hg_fanout_grad", "gradient 1 is null or not 16-byte aligned", d, arr(256, None), 2, 0, None)
    refused("hg_fanout_grad", "gradient 0 is null or not 16-byte aligned", d, arr(264, 256), 2, 1, None)
    refused("hg_fanout_grad", "G must be 16-byte aligned", off, ok2, 2, 0, None)


def test_parser_on_literal_declarations(native):
    """parse_header on text written here: pointers of any depth, each scalar type, (void), a declaration over three lines, one inside a block comment, an unknown type."""
    vp, u32, fl, c = native._vp, native._u32, native._fl, native._c
    got = native.parse_header("""
#define SOMETHING(x) 1
typedef void *nsig_stream_t;
int a(const float *const *x, void *, uint64_t seed, double, nsig_stream_t stream);   // int never(float x);
size_t b(void);
/* int inside_a_comment(uint32_t n);
   int another(float x); */
const char *c3(uint32_t n,
               int32_t k, int flag,
               float v, size_t bytes);
void *d(const void *host);
""")
    assert got == {"a": (c.c_int, [vp, vp, c.c_uint64, c.c_double, vp]), "b": (c.c_size_t, []),
                   "c3": (c.c_char_p, [u32, c.c_int32, c.c_int, fl, c.c_size_t]), "d": (vp, [vp])}
    with pytest.raises(native.NativeError, match=r"bad\(uint32_t n, long double v\).*'long double v'"):
        native.parse_header("int ok(float x);\nint bad(uint32_t n,\n        long double v);\n")
    with pytest.raises(native.NativeError, match=r"unsigned frob\(int x\);"):      # a return type outside the four: refused, not skipped
        native.parse_header("int ok(float x);\nunsigned frob(int x);\n")


def test_parser_finds_every_declaration(native):
    assert len(native.parse_header(open(os.path.join(ROOT, "include", "nerfsig.h")).read())) == len(_declared())
    assert set(native._RESTYPES) == set(native.SIGNATURES) == set(_declared())


def test_pinned_signatures_one_per_c_type(native):
    """Written out here, not derived: a 64-bit seed passed as 32 bits, or a double as a float, loads and runs."""
    c, vp, S, R = native._c, native._vp, native.SIGNATURES, native._RESTYPES
    assert S["rg_sample_rays"][13] is c.c_uint64 and len(S["rg_sample_rays"]) == 20
    assert S["wm_distort_draw"][1] is c.c_uint64 and S["wm_distort_draw"][0] is c.c_uint32
    assert S["opt_ema_update"] == [c.c_uint32, vp, vp, vp, vp, c.c_double, vp]
    assert S["hg_levels_scatter_adam"][7:11] == [vp, vp, vp, vp] and S["hg_levels_scatter_adam"][12:16] == [c.c_float] * 4
    assert S["field_fwd_multi"][4] is c.c_int and S["field_fwd_multi"][6] is c.c_uint32
    assert R["hg_planes_bytes"] is c.c_size_t and S["hg_planes_bytes"] == [c.c_uint32]
    assert R["nsig_last_error"] is c.c_char_p and S["nsig_last_error"] == []
    assert R["nsig_host_device_pointer"] is c.c_void_p and S["nsig_host_device_pointer"] == [vp]
    assert S["rm_march_train_scan_write_max_rays"] == [] and R["rm_march_train_scan_write_max_rays"] is c.c_int
    assert R["rg_sample_rays"] is c.c_int


def test_missing_header_fails_loudly(native, tmp_path):
    """The header is found relative to the package: a copy of the loader in a tree without include/nerfsig.h refuses to import, naming the path it looked at."""
    import importlib.util
    import shutil
    pkg = tmp_path / "pkg"
    pkg.mkdir()
    shutil.copy(native.__file__, pkg / "_native.py")
    spec = importlib.util.spec_from_file_location("_native_without_header", pkg / "_native.py")
    with pytest.raises(Exception) as e:
        spec.loader.exec_module(importlib.util.module_from_spec(spec))
    assert type(e.value).__name__ == "NativeError" and isinstance(e.value, RuntimeError)       # (the copy's own NativeError class)
    assert str(tmp_path / "pkg" / ".." / "include" / "nerfsig.h") in str(e.value)


def test_missing_library_fails_loudly(native, monkeypatch):
    monkeypatch.setattr(native, "_lib", None)
    monkeypatch.setattr(native, "_bound", {})
    monkeypatch.setattr(native, "LIB_PATH", "/nonexistent/libnerfsig.so")
    with pytest.raises(native.NativeError, match="no fallback"):
        native.fn("rm_morton3D")


def test_product_does_not_import_the_oracle():
    """Only tests/, smoke() and bench.py's cpu_baseline leg may use oracle/: the package never imports, links or
    dlopens it (comments may cite it)."""
    pkg = os.path.join(ROOT, "nerf_signature_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            path = os.path.join(dirpath, f)
            if f.endswith(".py"):
                for line in open(path):
                    code = line.split("#")[0]
                    assert not re.search(r"^\s*(from|import)\s+oracle\b", code), path
                    assert "liboracle" not in code and "raymarch_ref" not in code and "field_ref" not in code, path
            elif f.endswith((".hip", ".h")):
                for line in open(path):
                    assert not (line.lstrip().startswith("#include") and "oracle" in line), path
