"""CPU tests of binding.signatures(): the table of C signatures that lib() applies to libgrhip.so comes from
include/grhip.h alone.  No library and no device needed."""
import ast
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "grhip.h")
V = C.c_void_p


@pytest.fixture(scope="module")
def table(g):
    return g.binding.signatures()


def _stripped_header():
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", open(HEADER).read(), flags=re.S)
    return "\n".join(l for l in text.split("\n") if not l.lstrip().startswith("#"))


def test_one_entry_per_prototype(table):
    text = _stripped_header()
    names = re.findall(r"\bGRHIP_API\b[^;()]*?(\w+)\s*\([^()]*\)\s*;", text)
    assert len(names) == len(re.findall(r"\bGRHIP_API\b", text)) > 500
    assert len(set(names)) == len(names)
    assert sorted(table) == sorted(names)


def test_pinned_entries(table):
    assert table["grhip_fir_filter_create"] == (C.c_int, [V, V, C.c_int, V, C.c_size_t, C.c_int])
    assert table["grhip_agc_cc_rate"] == (C.c_float, [V])
    assert table["grhip_logpwrfft_c_sample_rate"] == (C.c_double, [V])
    assert table["grhip_fir_filter_destroy"] == (None, [V])
    assert table["grhip_strerror"] == (C.c_char_p, [C.c_int])
    assert table["grhip_last_error"] == (C.c_char_p, [])
    assert table["grhip_fir_filterNdec"] == (C.c_int, [V, V, V, C.c_ulong, C.c_uint])
    # (h, int n_streams, size_t n_samples, d_in, size_t, d_out, size_t, size_t *n_out, stream)
    assert table["grhip_pfb_arb_resampler_ccf_run_captures_device"] == \
        (C.c_int, [V, C.c_int, C.c_size_t, V, C.c_size_t, V, C.c_size_t, V, V])
    assert table["grhip_moving_average_ss_create"][1][2] is C.c_short
    assert table["grhip_head_create"][1][2] is C.c_ulonglong
    assert table["grhip_framer_sink_1_set_segment_items"][1][1] is C.c_longlong


def test_every_float_getter_is_typed(table):
    """the entries that return a float or a double: a getter read as an int would return garbage silently"""
    fl = sorted(n for n, (r, _) in table.items() if r in (C.c_float, C.c_double))
    for n in ("grhip_clock_recovery_mm_ff_mu", "grhip_fractional_interpolator_ff_interp_ratio",
              "grhip_logpwrfft_f_avg_alpha", "grhip_pwr_squelch_cc_threshold", "grhip_ctcss_squelch_ff_level",
              "grhip_agc2_ff_decay_rate"):
        assert n in fl
    text = _stripped_header()
    assert len(fl) == len(re.findall(r"\bGRHIP_API\s+(?:float|double)\s+\w+\s*\(", text))


def test_unmapped_type_names_the_declaration(g):
    with pytest.raises(ValueError, match="grhip_x"):
        g.binding.signatures("GRHIP_API int grhip_x(struct foo v);")
    with pytest.raises(ValueError, match="grhip_r"):
        g.binding.signatures("GRHIP_API struct foo grhip_r(int v);")
    with pytest.raises(ValueError, match="grhip_p"):
        g.binding.signatures("GRHIP_API float *grhip_p(int v);")


def test_every_token_must_parse(g):
    with pytest.raises(ValueError, match="grhip_y"):                            # no semicolon: two tokens, one prototype
        g.binding.signatures("GRHIP_API int grhip_y(int a)\nGRHIP_API int grhip_z(void);")
    with pytest.raises(ValueError, match="grhip_d"):                            # declared twice
        g.binding.signatures("GRHIP_API int grhip_d(void);\nGRHIP_API int grhip_d(int a);")


def test_split_prototype_comments_and_preprocessor_lines(g):
    text = """
    #define GRHIP_API __attribute__((visibility("default")))
    #define TWO_LINES(x) \\
        GRHIP_API x
    /* GRHIP_API int grhip_in_a_comment(void); */
    // GRHIP_API int grhip_in_a_line_comment(void);
    GRHIP_API int
    grhip_m(grhip_m *h, int a,        /* the count */
            const float *taps,
            unsigned long long n, double);
    GRHIP_API const char *grhip_s(void);
    """
    assert g.binding.signatures(text) == {"grhip_m": (C.c_int, [V, C.c_int, V, C.c_ulonglong, C.c_double]),
                                          "grhip_s": (C.c_char_p, [])}


def test_missing_header_is_an_import_error_with_the_path(g, monkeypatch):
    monkeypatch.setattr(g.binding, "_HEADER", os.path.join(ROOT, "include", "no_such_grhip.h"))
    with pytest.raises(ImportError, match="no_such_grhip.h"):
        g.binding.signatures()


def _binding_tree(g):
    return ast.parse(open(g.binding.__file__).read())


def test_signatures_are_assigned_in_one_function(g):
    """.argtypes / .restype are set in lib() and nowhere else in the binding"""
    def stores(root):
        return {id(e) for e in ast.walk(root) if isinstance(e, ast.Attribute) and e.attr in ("argtypes", "restype")
                and isinstance(e.ctx, ast.Store)}

    tree = _binding_tree(g)
    lib_fn = [n for n in ast.walk(tree) if isinstance(n, ast.FunctionDef) and n.name == "lib"]
    assert len(lib_fn) == 1
    assert len(stores(lib_fn[0])) == 2 and stores(tree) == stores(lib_fn[0])
    assert "setattr" not in open(g.binding.__file__).read()


def test_one_fn_and_no_private_float_helpers(g):
    defs = [n.name for n in ast.walk(_binding_tree(g)) if isinstance(n, ast.FunctionDef)]
    assert defs.count("_fn") == 1
    for gone in ("_getf", "_setf", "_get", "_set", "_raise_like_reference"):
        assert gone not in defs
