"""ctypes binding of libgrhip.so.  See include/grhip.h for the contract.

The header is also where every C signature comes from: signatures() parses its GRHIP_API prototypes and lib()
applies them to the loaded library once.  A new block needs no signature code here."""
import ctypes as C
import math
import os
import re

import numpy as np

__all__ = [
    "GrhipError", "lib", "lib_path", "strerror", "device_count", "set_default_mode",
    "MODE_FAST", "MODE_GENERIC", "MODE_FAST_VALU", "MODE_FAST_REFTAPS", "WORK_DONE",
    "fir_filter_ccf", "fir_filter_fff", "fir_filter_ccc", "fir_filter_fcc", "fir_filter_scc", "fir_filter_fsf",
    "fir_filter_with_buffer",
    "freq_xlating_fir_filter_ccc", "freq_xlating_fir_filter_ccf", "freq_xlating_fir_filter_fcf",
    "freq_xlating_fir_filter_fcc", "freq_xlating_fir_filter_scf", "freq_xlating_fir_filter_scc", "quadrature_demod_cf", "xlating_demod",
    "clock_recovery_mm_ff", "clock_recovery_mm_cc", "binary_slicer_fb", "correlate_access_code_bb", "pager_slicer_fb", "unpack_k_bits_bb", "framer_sink_1", "framer_sink_1_batch", "stream_to_streams", "streams_to_stream", "vector_to_streams", "stream_to_vector", "head",
    "fft_vcc", "fft_vfc", "fft_filter_ccc", "fft_filter_fff", "pfb_channelizer_ccf", "pfb_decimator_ccf", "pfb_arb_resampler_ccf", "pfb_arb_resampler_fff",
    "fractional_interpolator_ff", "fractional_interpolator_cc",
    "firdes_hilbert", "hilbert_fc", "filter_delay_fc", "goertzel_fc",
    "dc_blocker_ff", "dc_blocker_cc", "moving_average_ff", "moving_average_cc", "moving_average_ss", "moving_average_ii",
    "integrate_ff", "integrate_cc", "integrate_ss", "integrate_ii",
    "complex_to_mag_squared", "single_pole_iir_filter_ff", "nlog10_ff", "keep_one_in_n",
    "logpwrfft_c", "logpwrfft_f", "window_blackmanharris",
    "pwr_squelch_cc", "pwr_squelch_ff", "simple_squelch_cc", "ctcss_squelch_ff",
    "agc_cc", "agc_ff", "agc2_cc", "agc2_ff",
    "costas_loop_cc", "pll_freqdet_cf", "pll_refout_cc", "pll_carriertracking_cc",
    "fll_band_edge_cc", "fll_band_edge_taps", "firdes_root_raised_cosine",
    "pfb_clock_sync_ccf", "pfb_clock_sync_taps",
    "constellation", "constellation_bpsk", "constellation_qpsk", "constellation_dqpsk", "constellation_8psk",
    "constellation_calcdist", "constellation_psk", "constellation_rect", "psk_constellation", "qam_constellation",
    "gray_code", "invert_code", "constellation_decoder_cb", "diff_decoder_bb", "map_bb", "constellation_receiver_cb",
    "constellation_demod_cb",
    "packed_to_unpacked_bb", "unpacked_to_packed_bb", "GR_MSB_FIRST", "GR_LSB_FIRST", "diff_encoder_bb", "chunks_to_symbols_bc",
    "generic_mod", "psk_mod", "qam_mod", "bpsk_mod", "dbpsk_mod", "qpsk_mod", "dqpsk_mod",
    "scrambler_bb", "descrambler_bb", "additive_scrambler_bb", "crc32", "packet_maker", "packet_check", "random_mask_vec8",
    "default_access_code", "PACKET_JOB", "PACKET_REC",
    "frequency_modulator_fc", "bytes_to_syms", "char_to_float", "chunks_to_symbols_bf", "cpm_phase_response", "firdes_gaussian",
    "gmsk_mod_taps", "frequency_modulator_fc_tile", "cpmmod_bc", "gmskmod_bc", "gmsk_mod", "CPM_LRC", "CPM_LSRC", "CPM_LREC", "CPM_TFM", "CPM_GAUSSIAN",
    "fsm", "trellis_encoder_bb", "trellis_encoder_bs", "trellis_encoder_bi", "trellis_encoder_ss", "trellis_encoder_si",
    "trellis_encoder_ii", "trellis_metrics_s", "trellis_metrics_i", "trellis_metrics_f", "trellis_metrics_c",
    "trellis_constellation_metrics_cf", "trellis_viterbi_b", "trellis_viterbi_s", "trellis_viterbi_i",
    "trellis_viterbi_combined_sb", "trellis_viterbi_combined_ss", "trellis_viterbi_combined_si", "trellis_viterbi_combined_ib",
    "trellis_viterbi_combined_is", "trellis_viterbi_combined_ii", "trellis_viterbi_combined_fb", "trellis_viterbi_combined_fs",
    "trellis_viterbi_combined_fi", "trellis_viterbi_combined_cb", "trellis_viterbi_combined_cs", "trellis_viterbi_combined_ci",
    "TRELLIS_EUCLIDEAN", "TRELLIS_HARD_SYMBOL", "TRELLIS_HARD_BIT",
    "iir_filter_ffd", "fm_deemph", "fm_deemph_taps", "firdes_low_pass", "fm_demod_cf", "nbfm_rx",
    "remez", "optfir_low_pass", "optfir_high_pass", "optfir_band_pass", "optfir_band_reject", "optfir_spec",
    "complex_to_mag", "am_demod_cf", "demod_10k0a3e_cf", "demod_20k0f3e_cf", "demod_200kf3e_cf",
    "WIN_HAMMING", "WIN_HANN", "WIN_BLACKMAN", "WIN_RECTANGULAR", "WIN_KAISER", "WIN_BLACKMAN_hARRIS",
    "interp_fir_filter_ccf", "interp_fir_filter_fff", "interp_fir_filter_ccc",
    "rational_resampler_base_ccf", "rational_resampler_base_fff", "rational_resampler_base_ccc",
    "rational_resampler_ccf", "rational_resampler_fff", "rational_resampler_ccc", "design_filter",
    "pfb_interpolator_ccf", "pfb_synthesis_filterbank_ccf", "dmr_chain", "run_sync_block",
]

MODE_FAST = 0
MODE_GENERIC = 1
MODE_FAST_VALU = 2     # FAST without the matrix cores (vector FMAs only)
MODE_FAST_REFTAPS = 3  # FAST + the reference's tap-angle quantisation reproduced by freq_xlating's matrix-core engine
WORK_DONE = 0x7fffffff  # GRHIP_WORK_DONE: not an error, not an item count

_HERE = os.path.dirname(os.path.abspath(__file__))
_HEADER = os.path.join(_HERE, "..", "include", "grhip.h")      # where the Makefile finds it too
_LIB = None


class GrhipError(RuntimeError):
    def __init__(self, code, detail=""):
        self.code = code
        RuntimeError.__init__(self, "grhip error %d (%s): %s" % (code, strerror(code), detail))


# ----------------------------------------------------------------------------
# the C signatures, read from include/grhip.h
# ----------------------------------------------------------------------------
_CTYPES = {"int": C.c_int, "unsigned": C.c_uint, "short": C.c_short, "long long": C.c_longlong,
           "unsigned long": C.c_ulong, "unsigned long long": C.c_ulonglong, "size_t": C.c_size_t,
           "float": C.c_float, "double": C.c_double}
_PROTOTYPE = re.compile(r"GRHIP_API\s+([\w\s*]+?)(\w+)\s*\(([^()]*)\)\s*;")


def _ctype(text, decl, returned=False):
    """the ctypes twin of one parameter (type and optional name) or of a return type"""
    words = [w for w in text.replace("*", " * ").split() if w != "const"]
    if "*" in words:                            # every pointer parameter travels as an address
        if not returned:
            return C.c_void_p
        if words == ["char", "*"]:
            return C.c_char_p
    elif returned and words == ["void"]:
        return None
    else:
        for t in [words] if returned else [words, words[:-1]]:
            if " ".join(t) in _CTYPES:
                return _CTYPES[" ".join(t)]
    raise ValueError("grhip.h: no ctypes mapping for '%s' in: %s" % (" ".join(text.split()), decl))


def signatures(header_text=None):
    """{name: (restype, [argtypes])} of every GRHIP_API prototype of include/grhip.h (or of header_text).  Pure: it
    does not load the library.  A GRHIP_API that does not parse, or a type without a mapping, is an error."""
    if header_text is None:
        try:
            with open(_HEADER) as f:
                header_text = f.read()
        except OSError:
            raise ImportError("the C header of libgrhip.so is missing: %s" % os.path.normpath(_HEADER))
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", header_text, flags=re.S)
    text = re.sub(r"^[ \t]*#(?:[^\n]*\\\n)*[^\n]*", "", text, flags=re.M)
    table = {}
    for m in re.finditer(r"\bGRHIP_API\b", text):
        decl = " ".join(text[m.start():].partition(";")[0].split()) + ";"
        p = _PROTOTYPE.match(text, m.start())
        if p is None or p.group(2) in table:
            raise ValueError("grhip.h: not one well-formed prototype: %s" % decl)
        ret, name, params = p.groups()
        params = [a for a in params.split(",") if a.split() not in ([], ["void"])]
        table[name] = (_ctype(ret, decl, True), [_ctype(a, decl) for a in params])
    return table


def lib_path():
    # GRHIP_LIB: load another build of the same library (diagnostic builds only)
    return os.environ.get("GRHIP_LIB") or os.path.join(_HERE, "libgrhip.so")


def lib():
    """Load libgrhip.so (built in-tree by `make -C gnuradio-3.5.0-dmr_amd` /
    __graft_entry__.build()).  Fails loudly when it is missing."""
    global _LIB
    if _LIB is None:
        p = lib_path()
        # One HIP runtime per process: PyTorch-ROCm bundles its own libamdhip64
        # with the same SONAME.  If torch is going to be used for device memory /
        # streams / torch.distributed, it must be the copy that gets loaded first,
        # otherwise torch later reports "No HIP GPUs are available".
        if os.environ.get("GRHIP_NO_TORCH_PRELOAD") is None:
            try:
                import torch  # noqa: F401
            except Exception:
                pass
        if not os.path.exists(p):
            raise ImportError("libgrhip.so not built (%s): run __graft_entry__.build(); "
                              "there is no CPU fallback" % p)
        L = C.CDLL(p)
        # the one place that sets a signature: every entry gets the header's, before anything can call it
        for name, (restype, argtypes) in signatures().items():
            f = getattr(L, name)
            f.restype, f.argtypes = restype, argtypes
        _LIB = L
    return _LIB


def strerror(code):
    try:
        return lib().grhip_strerror(int(code)).decode()
    except Exception:
        return "?"


def _check(rc):
    """a negative status becomes a GrhipError (a RuntimeError, the type the reference's SWIG layer surfaces for the
    same preconditions: gnuradio-core/src/lib/swig/gnuradio.i:33-44)"""
    if rc < 0:
        raise GrhipError(rc, lib().grhip_last_error().decode())
    return rc


def device_count():
    n = C.c_int(0)
    rc = lib().grhip_device_count(C.byref(n))
    if rc < 0:
        return 0
    return n.value


def set_default_mode(mode):
    _check(lib().grhip_set_default_mode(int(mode)))


def _ptr(a):
    return C.c_void_p(a.ctypes.data)


def _devptr(t):
    """accept an int address or anything with data_ptr() (torch tensor)"""
    if t is None:
        return C.c_void_p(0)
    if hasattr(t, "data_ptr"):
        return C.c_void_p(t.data_ptr())
    return C.c_void_p(int(t))


def _stream(s):
    if s is None:
        return C.c_void_p(0)
    if hasattr(s, "cuda_stream"):
        return C.c_void_p(s.cuda_stream)
    return C.c_void_p(int(s))


class _Block(object):
    """one C handle.  Its entries are grhip_<_name>_<entry>; what most blocks share is spelled once here.

    A block whose host work takes streams x n steps back to back (StreamBlock::host_work in csrc/stream_block.h) says
    so in five attributes, any of which may be set per instance or be a property, and gets its checks and buffers from
    _work_in and _work_out, or the whole call from _stream_work."""
    _name = None
    _in = None              # dtype of the input items, cast to it ...
    _view = False           # ... or True: the input's own bytes, whatever its dtype
    _out = None             # dtype of the (first) output
    _per_in = 1             # items in per step and stream
    _per_out = 1            # items out per step and stream

    def __init__(self):
        self._h = C.c_void_p(0)
        self._streams = 1

    def __del__(self):
        try:
            if self._h:
                self._fn("destroy")(self._h)
                self._h = C.c_void_p(0)
        except Exception:
            pass

    def _fn(self, name):
        return getattr(lib(), "grhip_%s_%s" % (self._name, name))

    def _create(self, *args):
        _check(self._fn("create")(C.byref(self._h), *args))

    def _call(self, name, *args):
        return _check(self._fn(name)(self._h, *args))

    def set_mode(self, mode):
        self._call("set_mode", int(mode))

    def set_streams(self, nstreams):
        """work / work_device then take nstreams streams back to back, each of the item count they are given; restarts
        every stream from the block's initial state"""
        self._call("set_streams", int(nstreams))
        self._streams = int(nstreams)

    def work_device(self, n, d_in, d_out, stream=None):
        """work on device buffers (addresses or tensors), queued on `stream`"""
        return self._call("work_device", int(n), _devptr(d_in), _devptr(d_out), _stream(stream))

    def _stream_value(self, name, ctype, stream):
        """one value of one stream, which the entry `name` hands back through an out-parameter"""
        v = ctype(0)
        self._call(name, int(stream), C.byref(v))
        return v.value

    def _work_in(self, input_items, n=None):
        """(x, n): the input flat and contiguous, and the steps it is good for (all it holds where n is None)"""
        if self._view:
            x = np.ascontiguousarray(input_items).view(np.uint8).reshape(-1)
        else:
            x = np.ascontiguousarray(input_items, dtype=self._in).reshape(-1)
        n = len(x) // (self._streams * self._per_in) if n is None else int(n)
        if len(x) < n * self._streams * self._per_in:
            raise ValueError("work needs %d items, got %d" % (n * self._streams * self._per_in, len(x)))
        return x, n

    def _work_out(self, n, optional=(), wanted=False):
        """(pointers, arrays) of the outputs of n steps: the _out array and, where wanted, one array per dtype in
        `optional` (null pointers otherwise).  Every pointer is valid for n == 0 too; the arrays are cut to the items."""
        m = n * self._streams * self._per_out
        bufs = [np.zeros(max(m, 1), dtype=d) for d in [self._out] + (list(optional) if wanted else [])]
        nulls = [C.c_void_p(0)] * (0 if wanted else len(optional))
        return [_ptr(b) for b in bufs] + nulls, [b[:m] for b in bufs]

    def _stream_work(self, input_items, n, optional=(), wanted=False):
        """the work entry between the two: the _out array, or the tuple of it and the optional outputs where wanted"""
        x, n = self._work_in(input_items, n)
        ptrs, outs = self._work_out(n, optional, wanted)
        self._call("work", n, _ptr(x), *ptrs)
        return tuple(outs) if wanted else outs[0]


class _stream_block(_Block):
    """the blocks whose work is nothing but that contract and which keep no history.  A family that names the count
    otherwise, or takes it first, keeps a work of its own that hands over to _stream_work."""

    def history(self):
        return 1

    def work(self, input_items, n=None):
        return self._stream_work(input_items, n)


# ----------------------------------------------------------------------------
# gr.fir_filter_XXX  (filter/gr_fir_filter_XXX.i.t:28-41)
# ----------------------------------------------------------------------------
class _fir_filter(_Block):
    _name = "fir_filter"
    _kind = None
    _in = np.complex64
    _out = np.complex64
    _tap = np.float32

    def __init__(self, decimation, taps, device=0):
        _Block.__init__(self)
        t = np.ascontiguousarray(taps, dtype=self._tap)
        self._create(self._kind.encode(), int(decimation), _ptr(t), len(t), int(device))

    def set_taps(self, taps):
        t = np.ascontiguousarray(taps, dtype=self._tap)
        self._call("set_taps", _ptr(t), len(t))

    def history(self):
        return self._call("history")

    def decimation(self):
        return self._call("decimation")

    def work(self, noutput_items, input_items):
        """input_items: numpy array with history()-1 old items in front."""
        x = np.ascontiguousarray(input_items, dtype=self._in)
        need = noutput_items * self.decimation() + self.history() - 1
        if len(x) < need:
            raise ValueError("work needs %d input items, got %d" % (need, len(x)))
        out = np.zeros(noutput_items, dtype=self._out)
        n = self._call("work", int(noutput_items), _ptr(x), _ptr(out))
        return out[:n]

    def filterNdec(self, x, n, decimate):
        x = np.ascontiguousarray(x, dtype=self._in)
        out = np.zeros(n, dtype=self._out)
        _check(lib().grhip_fir_filterNdec(self._h, _ptr(out), _ptr(x), n, decimate))
        return out


class fir_filter_with_buffer(_Block):
    """gri_fir_filter_with_buffer_{ccf,ccc,fff}: the FIR kernel object that keeps its own delay line"""
    _name = "fir_filter_with_buffer"

    def __init__(self, kind, taps, device=0):
        _Block.__init__(self)
        self.kind = kind
        self._tap = np.complex64 if kind == "ccc" else np.float32
        self._io = np.float32 if kind == "fff" else np.complex64
        t = np.ascontiguousarray(taps, dtype=self._tap)
        self._create(kind.encode(), _ptr(t), len(t), int(device))

    def set_taps(self, taps):
        t = np.ascontiguousarray(taps, dtype=self._tap)
        self._call("set_taps", _ptr(t), len(t))

    def ntaps(self):
        return self._call("ntaps")

    def filterNdec(self, x, n, decimate=1):
        x = np.ascontiguousarray(x, dtype=self._io)
        if len(x) < n * decimate:
            raise ValueError("filterNdec needs %d items" % (n * decimate))
        out = np.zeros(n, dtype=self._io)
        self._call("filterNdec", _ptr(out), _ptr(x), n, decimate)
        return out

    def filterN(self, x, n):
        return self.filterNdec(x, n, 1)

    def filterNdec_device(self, d_out, d_in, n, decimate=1, stream=None):
        self._call("filterNdec_device", _devptr(d_out), _devptr(d_in), n, decimate, _stream(stream))


class fir_filter_ccf(_fir_filter):
    _kind = "ccf"


class fir_filter_fff(_fir_filter):
    _kind = "fff"
    _in = np.float32
    _out = np.float32


class fir_filter_ccc(_fir_filter):
    _kind = "ccc"
    _tap = np.complex64


class fir_filter_fcc(_fir_filter):
    """gr.fir_filter_fcc: float in, complex out, complex taps"""
    _kind = "fcc"
    _in = np.float32
    _tap = np.complex64


class fir_filter_scc(_fir_filter):
    """gr.fir_filter_scc: short in, complex out, complex taps"""
    _kind = "scc"
    _in = np.int16
    _tap = np.complex64


class fir_filter_fsf(_fir_filter):
    """gr.fir_filter_fsf: float in, short out, float taps"""
    _kind = "fsf"
    _in = np.float32
    _out = np.int16


# ----------------------------------------------------------------------------
# gr.freq_xlating_fir_filter_{ccc,ccf,fcf,fcc,scf,scc}: one C handle for the family
# (filter/gr_freq_xlating_fir_filter_XXX.i.t)
# ----------------------------------------------------------------------------
class _freq_xlating_fir_filter(_Block):
    _name = "freq_xlating_fir_filter"
    _kind = None
    _in = np.complex64
    _tap = np.float32

    def __init__(self, decimation, taps, center_freq, sampling_freq, device=0):
        _Block.__init__(self)
        t = np.ascontiguousarray(taps, dtype=self._tap)
        self._decim = int(decimation)
        kind = [self._kind.encode()] if self._kind else []      # the _ccc entry takes no kind
        self._create(*kind, self._decim, _ptr(t), len(t), float(center_freq), float(sampling_freq), int(device))

    def set_center_freq(self, center_freq):
        self._call("set_center_freq", float(center_freq))

    def set_taps(self, taps):
        t = np.ascontiguousarray(taps, dtype=self._tap)
        self._call("set_taps", _ptr(t), len(t))

    def reset(self):
        self._call("reset")

    def history(self):
        return self._call("history")

    def decimation(self):
        return self._decim

    def work(self, noutput_items, input_items):
        x = np.ascontiguousarray(input_items, dtype=self._in)
        need = noutput_items * self._decim + self.history() - 1
        if len(x) < need:
            raise ValueError("work needs %d input items, got %d" % (need, len(x)))
        out = np.zeros(noutput_items, dtype=np.complex64)
        n = self._call("work", int(noutput_items), _ptr(x), _ptr(out))
        return out[:n]


class freq_xlating_fir_filter_ccc(_freq_xlating_fir_filter):
    # the family handle of kind "ccc" behind gr.freq_xlating_fir_filter_ccc's own C entries
    _name = "freq_xlating_fir_filter_ccc"
    _tap = np.complex64


class freq_xlating_fir_filter_ccf(_freq_xlating_fir_filter):
    _kind = "ccf"


class freq_xlating_fir_filter_fcf(_freq_xlating_fir_filter):
    _kind = "fcf"
    _in = np.float32


class freq_xlating_fir_filter_fcc(_freq_xlating_fir_filter):
    _kind = "fcc"
    _in = np.float32
    _tap = np.complex64


class freq_xlating_fir_filter_scf(_freq_xlating_fir_filter):
    _kind = "scf"
    _in = np.int16


class freq_xlating_fir_filter_scc(_freq_xlating_fir_filter):
    _kind = "scc"
    _in = np.int16
    _tap = np.complex64


# ----------------------------------------------------------------------------
# gr.quadrature_demod_cf
# ----------------------------------------------------------------------------
class quadrature_demod_cf(_Block):
    _name = "quadrature_demod_cf"

    def __init__(self, gain, device=0):
        _Block.__init__(self)
        self._create(float(gain), int(device))

    def history(self):
        return 2

    def decimation(self):
        return 1

    def work(self, noutput_items, input_items):
        x = np.ascontiguousarray(input_items, dtype=np.complex64)
        if len(x) < noutput_items + 1:
            raise ValueError("work needs %d input items" % (noutput_items + 1))
        out = np.zeros(noutput_items, dtype=np.float32)
        n = self._call("work", int(noutput_items), _ptr(x), _ptr(out))
        return out[:n]


# ----------------------------------------------------------------------------
# fused hier block xlating -> quad_demod
# ----------------------------------------------------------------------------
class xlating_demod(_Block):
    _name = "xlating_demod"

    def __init__(self, decimation, taps, center_freq, sampling_freq, gain, device=0):
        _Block.__init__(self)
        t = np.ascontiguousarray(taps, dtype=np.complex64)
        self._decim = int(decimation)
        self._create(self._decim, _ptr(t), len(t), float(center_freq), float(sampling_freq), float(gain), int(device))

    def reset(self):
        self._call("reset")

    def history(self):
        return self._call("history")

    def decimation(self):
        return self._decim

    def work(self, noutput_items, input_items):
        x = np.ascontiguousarray(input_items, dtype=np.complex64)
        need = noutput_items * self._decim + self.history() - 1
        if len(x) < need:
            raise ValueError("work needs %d input items, got %d" % (need, len(x)))
        out = np.zeros(noutput_items, dtype=np.float32)
        n = self._call("work", int(noutput_items), _ptr(x), _ptr(out))
        return out[:n]

    def run_captures_device(self, n_streams, n_samples, d_in, in_stride_items, d_out, out_stride_items,
                            stream=None):
        """n_streams fresh-state captures (no history in front) in one launch"""
        return self._call("run_captures_device", int(n_streams), int(n_samples), _devptr(d_in), int(in_stride_items),
                          _devptr(d_out), int(out_stride_items), _stream(stream))


# ----------------------------------------------------------------------------
# digital.clock_recovery_mm_ff
# ----------------------------------------------------------------------------
class clock_recovery_mm_ff(_Block):
    _name = "clock_recovery_mm_ff"

    def __init__(self, omega, gain_omega, mu, gain_mu, omega_relative_limit, device=0):
        _Block.__init__(self)
        self._create(omega, gain_omega, mu, gain_mu, omega_relative_limit, int(device))

    def forecast(self, noutput_items):
        return self._call("forecast", int(noutput_items))

    def general_work(self, noutput_items, input_items):
        """returns (out, consumed)"""
        x = np.ascontiguousarray(input_items, dtype=np.float32)
        out = np.zeros(max(int(noutput_items), 1), dtype=np.float32)
        consumed = C.c_int(0)
        n = self._call("general_work", int(noutput_items), len(x), _ptr(x), _ptr(out), C.byref(consumed))
        return out[:n].copy(), consumed.value

    def general_work_device(self, noutput_items, ninput_items, d_in, d_out, d_counts, stream=None):
        return self._call("general_work_device", int(noutput_items), int(ninput_items), _devptr(d_in), _devptr(d_out),
                          _devptr(d_counts), _stream(stream))

    # the getters return the float itself, not a status
    def mu(self):
        return self._fn("mu")(self._h)

    def omega(self):
        return self._fn("omega")(self._h)

    def gain_mu(self):
        return self._fn("gain_mu")(self._h)

    def gain_omega(self):
        return self._fn("gain_omega")(self._h)

    def set_gain_mu(self, v):
        self._call("set_gain_mu", float(v))

    def set_gain_omega(self, v):
        self._call("set_gain_omega", float(v))

    def set_mu(self, v):
        self._call("set_mu", float(v))

    def set_omega(self, v):
        self._call("set_omega", float(v))


# ----------------------------------------------------------------------------
# digital.binary_slicer_fb / digital.correlate_access_code_bb
# ----------------------------------------------------------------------------
class binary_slicer_fb(_Block):
    _name = "binary_slicer_fb"

    def __init__(self, device=0):
        _Block.__init__(self)
        self._create(int(device))

    def history(self):
        return 1

    def decimation(self):
        return 1

    def work(self, noutput_items, input_items):
        x = np.ascontiguousarray(input_items, dtype=np.float32)
        out = np.zeros(noutput_items, dtype=np.uint8)
        n = self._call("work", int(noutput_items), _ptr(x), _ptr(out))
        return out[:n]


class pager_slicer_fb(_Block):
    """pager.slicer_fb(alpha): DC-tracking 4-level slicer (gr-pager/lib/pager_slicer_fb.cc)"""
    _name = "pager_slicer_fb"

    def __init__(self, alpha, device=0):
        _Block.__init__(self)
        self._create(float(alpha), int(device))

    def history(self):
        return 1

    def decimation(self):
        return 1

    def work(self, noutput_items, input_items):
        x = np.ascontiguousarray(input_items, dtype=np.float32)
        out = np.zeros(noutput_items, dtype=np.uint8)
        n = self._call("work", int(noutput_items), _ptr(x), _ptr(out))
        return out[:n]

    def dc_offset(self):
        v = C.c_float(0)
        self._call("dc_offset", C.byref(v))
        return np.float32(v.value)


class unpack_k_bits_bb(_Block):
    """gr.unpack_k_bits_bb(k): k output bytes (one bit each, MSB first) per input byte"""
    _name = "unpack_k_bits_bb"

    def __init__(self, k, device=0):
        _Block.__init__(self)
        self._create(int(k), int(device))
        self.k = int(k)

    def interpolation(self):
        return self.k

    def work(self, noutput_items, input_items):
        x = np.ascontiguousarray(input_items, dtype=np.uint8)
        out = np.zeros(noutput_items, dtype=np.uint8)
        n = self._call("work", int(noutput_items), _ptr(x), _ptr(out))
        return out[:n]


class clock_recovery_mm_cc(_Block):
    """digital.clock_recovery_mm_cc(omega, gain_omega, mu, gain_mu, omega_relative_limit)"""
    _name = "clock_recovery_mm_cc"

    def __init__(self, omega, gain_omega, mu, gain_mu, omega_relative_limit, device=0):
        _Block.__init__(self)
        self._create(omega, gain_omega, mu, gain_mu, omega_relative_limit, int(device))

    def forecast(self, noutput_items):
        return self._call("forecast", int(noutput_items))

    def history(self):
        return self._call("history")

    def _out_float(self, name):
        v = C.c_float(0)
        self._call(name, C.byref(v))
        return np.float32(v.value)

    def mu(self): return self._out_float("mu")
    def omega(self): return self._out_float("omega")
    def gain_mu(self): return self._out_float("gain_mu")
    def gain_omega(self): return self._out_float("gain_omega")
    def set_mu(self, v): self._call("set_mu", float(v))
    def set_omega(self, v): self._call("set_omega", float(v))
    def set_gain_mu(self, v): self._call("set_gain_mu", float(v))
    def set_gain_omega(self, v): self._call("set_gain_omega", float(v))

    def general_work(self, noutput_items, input_items, want_error=False):
        """returns (out[:n], err[:n] or None, consumed)"""
        x = np.ascontiguousarray(input_items, dtype=np.complex64)
        out = np.zeros(max(noutput_items, 1), dtype=np.complex64)
        err = np.zeros(max(noutput_items, 1), dtype=np.float32) if want_error else None
        consumed = C.c_int(0)
        n = self._call("general_work", int(noutput_items), len(x), _ptr(x), _ptr(out),
                       _ptr(err) if want_error else None, C.byref(consumed))
        return out[:n], (err[:n] if want_error else None), consumed.value

    def general_work_device(self, noutput_items, ninput_items, d_in, d_out, d_err=None, stream=None):
        """device buffers (d_err may be None: no error output, clip limit 1.0); returns (produced, consumed)"""
        consumed = C.c_int(0)
        n = self._call("general_work_device", int(noutput_items), int(ninput_items), _devptr(d_in), _devptr(d_out),
                       _devptr(d_err), C.byref(consumed), _stream(stream))
        return n, consumed.value


class _copy_adapter(_Block):
    _name = "copy_adapter"          # stream_to_vector and head have a create entry each and share the rest

    def work(self, noutput_items, input_items):
        x = np.ascontiguousarray(input_items)
        out = np.zeros(max(noutput_items, 1) * self.out_bytes, dtype=np.uint8)
        n = self._call("work", int(noutput_items), _ptr(x), _ptr(out))   # negative: always an error
        if n == WORK_DONE:
            return None
        return out[:n * self.out_bytes].view(x.dtype)

    def work_device(self, noutput_items, d_in, d_out, stream=None):
        n = _Block.work_device(self, noutput_items, d_in, d_out, stream)
        return None if n == WORK_DONE else n


class stream_to_vector(_copy_adapter):
    """gr.stream_to_vector(item_size, nitems_per_block)"""

    def __init__(self, item_size, nitems_per_block, device=0):
        _Block.__init__(self)
        _check(lib().grhip_stream_to_vector_create(C.byref(self._h), int(item_size), int(nitems_per_block), int(device)))
        self.out_bytes = int(item_size) * int(nitems_per_block)


class head(_copy_adapter):
    """gr.head(sizeof_stream_item, nitems): work() / work_device() return None (WORK_DONE) once nitems have passed"""

    def __init__(self, sizeof_stream_item, nitems, device=0):
        _Block.__init__(self)
        _check(lib().grhip_head_create(C.byref(self._h), int(sizeof_stream_item), int(nitems), int(device)))
        self.out_bytes = int(sizeof_stream_item)

    def reset(self):
        _check(lib().grhip_head_reset(self._h))


class framer_sink_1_batch(_Block):
    """multi-capture gr.framer_sink_1: run_device() frames n_streams item streams in one go (every stream from
    the search state); messages() -> [[(whitener_offset, payload bytes), ...] per stream]"""
    _name = "framer_sink_1_batch"

    def __init__(self, n_streams, max_items_per_stream, device=0):
        _Block.__init__(self)
        self._create(int(n_streams), int(max_items_per_stream), int(device))
        self.n_streams = int(n_streams)

    def run_device(self, d_in, stream_stride_items, d_nitems, n_items_max, stream=None, nitems_stride=1):
        self._call("run_device", _devptr(d_in), int(stream_stride_items), _devptr(d_nitems), int(nitems_stride),
                   int(n_items_max), _stream(stream))

    def device_view(self):
        """where the last run_device left its messages on the device, as packet_check.work_device takes them:
        dict(d_recs, rec_stride, d_counts, count_stride_words, d_pool, pool_stride).  Addresses and strides are fixed at
        create; their contents are the last run's until the next one"""
        recs, counts, pool = C.c_void_p(0), C.c_void_p(0), C.c_void_p(0)
        rs, ps, cs = C.c_longlong(0), C.c_longlong(0), C.c_int(0)
        self._call("device_view", C.byref(recs), C.byref(rs), C.byref(counts), C.byref(cs), C.byref(pool), C.byref(ps))
        return dict(d_recs=recs.value, rec_stride=rs.value, d_counts=counts.value, count_stride_words=cs.value,
                    d_pool=pool.value, pool_stride=ps.value)

    def messages(self, stream=None):
        self._call("fetch", _stream(stream))
        buf = np.zeros(4096, np.uint8)
        out = []
        for s in range(self.n_streams):
            msgs = []
            for i in range(self._call("count", s)):
                w = C.c_int(0)
                ln = self._call("get", s, i, C.byref(w), _ptr(buf), 4096)
                msgs.append((w.value, buf[:ln].tobytes()))
            out.append(msgs)
        return out


class framer_sink_1(_Block):
    """gr.framer_sink_1(msgq): header + payload extraction after the correlator's flag bit.
    The reference inserts gr.message objects into `msgq`; here work() / work_device() collect them
    and messages() returns (and removes) [(whitener_offset, payload bytes), ...] in order."""
    _name = "framer_sink_1"

    def __init__(self, device=0):
        _Block.__init__(self)
        self._create(int(device))

    def work(self, noutput_items, input_items):
        x = np.ascontiguousarray(input_items, dtype=np.uint8)
        return self._call("work", int(noutput_items), _ptr(x))

    def set_segment_items(self, items):
        """tuning: items per segment of the parallel walk of long calls (0 = automatic); results do not depend on it"""
        self._call("set_segment_items", int(items))

    def work_device(self, noutput_items, d_in, stream=None):
        return self._call("work_device", int(noutput_items), _devptr(d_in), _stream(stream))

    def messages(self, stream=None):
        n = self._call("message_count", _stream(stream))
        out = []
        while n > 0:
            k = min(n, 1 << 16)
            woff = np.zeros(k, dtype=np.int32)
            lens = np.zeros(k, dtype=np.int32)
            buf = np.zeros(k * 4096 if k < 64 else max(k * 256, 1 << 20), dtype=np.uint8)
            got = self._call("drain", k, _ptr(woff), _ptr(lens), _ptr(buf), buf.size)
            if got == 0:                                   # a single payload larger than the share of the buffer
                buf = np.zeros(4096, dtype=np.uint8)
                got = self._call("drain", 1, _ptr(woff), _ptr(lens), _ptr(buf), buf.size)
            ends = np.cumsum(lens[:got])
            raw = buf.tobytes()
            for i in range(got):
                out.append((int(woff[i]), raw[ends[i] - lens[i]:ends[i]]))
            n -= got
        return out


class _stream_adapter(_Block):
    _name = "stream_adapter"
    _split = 1

    def __init__(self, item_size, nstreams, device=0):
        _Block.__init__(self)
        self._create(self._split, int(item_size), int(nstreams), int(device))
        self.item_size, self.nstreams = int(item_size), int(nstreams)

    def _work(self, n, single, streams):
        arr = (C.c_void_p * self.nstreams)(*[s.ctypes.data for s in streams])
        return self._call("work", int(n), single.ctypes.data, arr)

    def work_device(self, n_items_per_stream, d_single, d_streams, stream_stride_items, stream=None):
        return self._call("work_device", int(n_items_per_stream), _devptr(d_single), _devptr(d_streams),
                          int(stream_stride_items), _stream(stream))


class stream_to_streams(_stream_adapter):
    """gr.stream_to_streams(item_size, nstreams): work(noutput_items, input) -> list of nstreams arrays"""
    _split = 1

    def work(self, noutput_items, input_items):
        x = np.ascontiguousarray(input_items)
        assert x.dtype.itemsize == self.item_size
        outs = [np.zeros(noutput_items, dtype=x.dtype) for _ in range(self.nstreams)]
        self._work(noutput_items, x, outs)
        return outs


class vector_to_streams(stream_to_streams):
    """gr.vector_to_streams(item_size, nstreams): item j of every input vector -> stream j (same data movement as
    stream_to_streams, general/gr_vector_to_streams.cc:45-70)"""


class streams_to_stream(_stream_adapter):
    """gr.streams_to_stream(item_size, nstreams): work(noutput_items, [inputs]) -> one array"""
    _split = 0

    def work(self, noutput_items, input_items):
        ins = [np.ascontiguousarray(a) for a in input_items]
        assert noutput_items % self.nstreams == 0 and ins[0].dtype.itemsize == self.item_size
        out = np.zeros(noutput_items, dtype=ins[0].dtype)
        self._work(noutput_items // self.nstreams, out, ins)
        return out


class correlate_access_code_bb(_Block):
    _name = "correlate_access_code_bb"

    def __init__(self, access_code, threshold, device=0):
        _Block.__init__(self)
        code = access_code.encode("latin-1") if isinstance(access_code, str) else bytes(access_code)
        self._create(code, len(code), int(threshold), int(device))

    def set_access_code(self, access_code):
        code = access_code.encode("latin-1") if isinstance(access_code, str) else bytes(access_code)
        rc = self._fn("set_access_code")(self._h, code, len(code))
        return rc == 0   # bool like the reference (digital_correlate_access_code_bb.cc:64-68)

    def history(self):
        return 1

    def decimation(self):
        return 1

    def work(self, noutput_items, input_items):
        x = np.ascontiguousarray(input_items, dtype=np.uint8)
        out = np.zeros(noutput_items, dtype=np.uint8)
        n = self._call("work", int(noutput_items), _ptr(x), _ptr(out))
        return out[:n]


# ----------------------------------------------------------------------------
# gr.fft_vcc
# ----------------------------------------------------------------------------
class fft_vcc(_Block):
    _name = "fft_vcc"

    def __init__(self, fft_size, forward, window, shift=False, device=0):
        _Block.__init__(self)
        w = np.ascontiguousarray(window if window is not None else [], dtype=np.float32)
        self.fft_size = int(fft_size)
        self._create(self.fft_size, int(bool(forward)), _ptr(w) if len(w) else None, len(w), int(bool(shift)),
                     int(device))

    def set_window(self, window):
        w = np.ascontiguousarray(window, dtype=np.float32)
        return bool(self._call("set_window", _ptr(w) if len(w) else None, len(w)))

    def work(self, noutput_items, input_items):
        """items are vectors: input_items has noutput_items*fft_size complex."""
        x = np.ascontiguousarray(input_items, dtype=np.complex64).reshape(-1)
        if len(x) < noutput_items * self.fft_size:
            raise ValueError("not enough input")
        out = np.zeros(noutput_items * self.fft_size, dtype=np.complex64)
        n = self._call("work", int(noutput_items), _ptr(x), _ptr(out))
        return out[:n * self.fft_size]


# ----------------------------------------------------------------------------
# gr.fft_filter_ccc / gr.fft_filter_fff / gr.fft_vfc
# ----------------------------------------------------------------------------
class _fft_filter(_Block):
    _dtype = None

    def __init__(self, decimation, taps, device=0):
        _Block.__init__(self)
        t = np.ascontiguousarray(taps, dtype=self._dtype)
        self._create(int(decimation), _ptr(t), len(t), int(device))

    def history(self):
        return 1

    def decimation(self):
        return self._call("decimation")

    def nsamples(self):
        """the block's output multiple"""
        return self._call("nsamples")

    def set_taps(self, taps):
        t = np.ascontiguousarray(taps, dtype=self._dtype)
        self._call("set_taps", _ptr(t), len(t))

    def work(self, noutput_items, input_items):
        x = np.ascontiguousarray(input_items, dtype=self._dtype)
        out = np.zeros(noutput_items, dtype=self._dtype)
        n = self._call("work", int(noutput_items), _ptr(x), _ptr(out))
        return out[:n]


class fft_filter_ccc(_fft_filter):
    """gr.fft_filter_ccc(decimation, taps): overlap-add fast convolution (history 1, output multiple nsamples)"""
    _name = "fft_filter_ccc"
    _dtype = np.complex64


class fft_filter_fff(_fft_filter):
    """gr.fft_filter_fff(decimation, taps): fast convolution of a float stream with float taps (history 1, output
    multiple nsamples); two consecutive blocks share one complex transform"""
    _name = "fft_filter_fff"
    _dtype = np.float32

    def work(self, noutput_items, input_items):
        x = np.ascontiguousarray(input_items, dtype=np.float32)
        if len(x) < noutput_items * self.decimation():
            raise ValueError("not enough input")
        return _fft_filter.work(self, noutput_items, x)


class fft_vfc(_Block):
    """gr.fft_vfc(fft_size, forward, window): items of fft_size floats in, fft_size complex out; forward only"""
    _name = "fft_vfc"

    def __init__(self, fft_size, forward, window, device=0):
        _Block.__init__(self)
        w = np.ascontiguousarray(window if window is not None else [], dtype=np.float32)
        self.fft_size = int(fft_size)
        self._create(self.fft_size, int(bool(forward)), _ptr(w) if len(w) else None, len(w), int(device))

    def set_window(self, window):
        w = np.ascontiguousarray(window, dtype=np.float32)
        return bool(self._call("set_window", _ptr(w) if len(w) else None, len(w)))

    def work(self, noutput_items, input_items):
        """items are vectors: input_items has noutput_items*fft_size floats."""
        x = np.ascontiguousarray(input_items, dtype=np.float32).reshape(-1)
        if len(x) < noutput_items * self.fft_size:
            raise ValueError("not enough input")
        out = np.zeros(noutput_items * self.fft_size, dtype=np.complex64)
        n = self._call("work", int(noutput_items), _ptr(x), _ptr(out))
        return out[:n * self.fft_size]


# ----------------------------------------------------------------------------
# gr.pfb_channelizer_ccf / gr.pfb_decimator_ccf
# ----------------------------------------------------------------------------
class pfb_channelizer_ccf(_Block):
    _name = "pfb_channelizer_ccf"

    def __init__(self, numchans, taps, oversample_rate=1, device=0):
        _Block.__init__(self)
        t = np.ascontiguousarray(taps, dtype=np.float32)
        self.numchans = int(numchans)
        self._create(self.numchans, _ptr(t), len(t), float(oversample_rate), int(device))

    def set_taps(self, taps):
        t = np.ascontiguousarray(taps, dtype=np.float32)
        self._call("set_taps", _ptr(t), len(t))

    def history(self):
        return self._call("history")

    def output_multiple(self):
        return self._call("output_multiple")

    def general_work(self, noutput_items, streams):
        """streams: list of numchans complex arrays each with history()-1 old
        items in front.  Returns (out[n, numchans], consumed)."""
        arrs = [np.ascontiguousarray(s, dtype=np.complex64) for s in streams]
        ptrs = (C.c_void_p * self.numchans)(*[a.ctypes.data for a in arrs])
        out = np.zeros((max(noutput_items, 1), self.numchans), dtype=np.complex64)
        consumed = C.c_int(0)
        n = self._call("general_work", int(noutput_items), ptrs, _ptr(out), C.byref(consumed))
        return out[:n], consumed.value

    def general_work_device(self, noutput_items, d_in, stream_stride_items, d_out, stream=None):
        return self._call("general_work_device", int(noutput_items), _devptr(d_in), int(stream_stride_items),
                          _devptr(d_out), _stream(stream))

    def hier_work_device(self, noutput_items, d_in, d_out, out_stride_items, stream=None):
        """blks2.pfb_channelizer_ccf (hier block) in one call: one interleaved stream in (taps_per_filter * numchans history
        items in front), numchans streams out (channel k at d_out + k * out_stride_items)"""
        return self._call("hier_work_device", int(noutput_items), _devptr(d_in), _devptr(d_out), int(out_stride_items),
                          _stream(stream))


class pfb_decimator_ccf(_Block):
    """gr.pfb_decimator_ccf(decim, taps, channel)"""
    _name = "pfb_decimator_ccf"

    def __init__(self, decim, taps, channel=0, device=0):
        _Block.__init__(self)
        t = np.ascontiguousarray(taps, dtype=np.float32)
        self.decim = int(decim)
        self._create(self.decim, _ptr(t), len(t), int(channel), int(device))

    def set_taps(self, taps):
        t = np.ascontiguousarray(taps, dtype=np.float32)
        self._call("set_taps", _ptr(t), len(t))

    def history(self):
        return self._call("history")

    def work(self, noutput_items, streams):
        arrs = [np.ascontiguousarray(s, dtype=np.complex64) for s in streams]
        ptrs = (C.c_void_p * self.decim)(*[a.ctypes.data for a in arrs])
        out = np.zeros(max(noutput_items, 1), dtype=np.complex64)
        n = self._call("work", int(noutput_items), ptrs, _ptr(out))
        return out[:n]

    def work_device(self, noutput_items, d_in, stream_stride_items, d_out, stream=None):
        return self._call("work_device", int(noutput_items), _devptr(d_in), int(stream_stride_items), _devptr(d_out),
                          _stream(stream))


# ----------------------------------------------------------------------------
# What the schedule-driven general_work blocks share (csrc/sched_block.h): their C entry points differ only in the
# block's name, their buffers only in the item type.  The resamplers below have the same entries.
# ----------------------------------------------------------------------------
class _sched_block(_Block):
    _dtype = None

    def history(self):
        return self._call("history")

    def forecast(self, noutput_items):
        return self._call("forecast", int(noutput_items))

    def general_work(self, noutput_items, input_items):
        """returns (out, consumed)"""
        x = np.ascontiguousarray(input_items, dtype=self._dtype)
        out = np.zeros(max(int(noutput_items), 1), dtype=self._dtype)
        consumed = C.c_int(0)
        n = self._call("general_work", int(noutput_items), len(x), _ptr(x), _ptr(out), C.byref(consumed))
        return out[:n].copy(), consumed.value

    def general_work_device(self, noutput_items, ninput_items, d_in, d_out, stream=None):
        """returns (produced, consumed); the outputs are in d_out once `stream` has run"""
        consumed = C.c_int(0)
        n = self._call("general_work_device", int(noutput_items), int(ninput_items), _devptr(d_in), _devptr(d_out),
                       C.byref(consumed), _stream(stream))
        return n, consumed.value

    def run_captures_device(self, n_streams, n_samples, d_in, in_stride_items, d_out, out_stride_items,
                            stream=None):
        """n_streams fresh-state captures in one launch; returns the outputs per capture.  d_out=None only returns
        that number."""
        n_out = C.c_size_t(0)
        self._call("run_captures_device", int(n_streams), int(n_samples), _devptr(d_in), int(in_stride_items),
                   _devptr(d_out), int(out_stride_items), C.byref(n_out), _stream(stream))
        return n_out.value

    def captures_nout(self, n_samples):
        """outputs of one fresh-state capture of n_samples items"""
        return self.run_captures_device(1, n_samples, None, n_samples, None, 0)


# ----------------------------------------------------------------------------
# gr.pfb_arb_resampler_ccf / gr.pfb_arb_resampler_fff  (filter/gr_pfb_arb_resampler_ccf.i)
# ----------------------------------------------------------------------------
class _pfb_arb_resampler(_sched_block):
    def __init__(self, rate, taps, filter_size=32, device=0):
        _Block.__init__(self)
        t = np.ascontiguousarray(taps, dtype=np.float32)
        self._create(float(rate), _ptr(t), len(t), int(filter_size), int(device))

    def set_rate(self, rate):
        self._call("set_rate", float(rate))

    def taps_per_filter(self):
        return self._call("taps_per_filter")

    # the two overrides below only carry this block's wording of the docstrings
    def general_work(self, noutput_items, input_items):
        """returns (out, consumed); input_items carries the history in front"""
        return _sched_block.general_work(self, noutput_items, input_items)

    def run_captures_device(self, n_streams, n_samples, d_in, in_stride_items, d_out, out_stride_items,
                            stream=None):
        """n_streams fresh-state captures (no history in front) in one launch; returns the outputs per capture.
        d_out=None only returns that number."""
        return _sched_block.run_captures_device(self, n_streams, n_samples, d_in, in_stride_items, d_out,
                                                out_stride_items, stream)


class pfb_arb_resampler_ccf(_pfb_arb_resampler):
    """gr.pfb_arb_resampler_ccf(rate, taps, filter_size=32)"""
    _name = "pfb_arb_resampler_ccf"
    _dtype = np.complex64


class pfb_arb_resampler_fff(_pfb_arb_resampler):
    """gr.pfb_arb_resampler_fff(rate, taps, filter_size=32)"""
    _name = "pfb_arb_resampler_fff"
    _dtype = np.float32


# ----------------------------------------------------------------------------
# gr.fractional_interpolator_ff / gr.fractional_interpolator_cc  (filter/gr_fractional_interpolator_ff.i)
# ----------------------------------------------------------------------------
class _fractional_interpolator(_sched_block):
    def __init__(self, phase_shift, interp_ratio, device=0):
        _Block.__init__(self)
        self._create(float(phase_shift), float(interp_ratio), int(device))

    def mu(self):
        return self._fn("mu")(self._h)

    def interp_ratio(self):
        return self._fn("interp_ratio")(self._h)

    def set_mu(self, mu):
        self._call("set_mu", float(mu))

    def set_interp_ratio(self, interp_ratio):
        self._call("set_interp_ratio", float(interp_ratio))


class fractional_interpolator_ff(_fractional_interpolator):
    """gr.fractional_interpolator_ff(phase_shift, interp_ratio)"""
    _name = "fractional_interpolator_ff"
    _dtype = np.float32


class fractional_interpolator_cc(_fractional_interpolator):
    """gr.fractional_interpolator_cc(phase_shift, interp_ratio)"""
    _name = "fractional_interpolator_cc"
    _dtype = np.complex64


# ----------------------------------------------------------------------------
# gr.firdes.hilbert, gr.hilbert_fc, gr.filter_delay_fc, gr.goertzel_fc  (general/gr_firdes.i, filter/gr_hilbert_fc.i,
# filter/gr_filter_delay_fc.i, filter/gr_goertzel_fc.i)
# ----------------------------------------------------------------------------
WIN_HAMMING, WIN_HANN, WIN_BLACKMAN, WIN_RECTANGULAR, WIN_KAISER, WIN_BLACKMAN_hARRIS = range(6)


def firdes_hilbert(ntaps, window=WIN_RECTANGULAR, beta=6.76):
    """gr.firdes.hilbert(ntaps, window, beta): host arithmetic only, no device needed.  WIN_RECTANGULAR gives the
    Hamming-windowed taps, as the reference's window() does (its case has no break)."""
    ntaps = int(ntaps)
    if ntaps < 0 or ntaps > (1 << 24):
        raise ValueError("ntaps out of range")
    out = np.zeros(max(ntaps, 1), dtype=np.float32)
    _check(lib().grhip_firdes_hilbert(ntaps, int(window), float(beta), _ptr(out)))
    return out[:ntaps]


class _analytic(_Block):
    def history(self):
        return self._call("history")

    def decimation(self):
        return 1

    def ntaps(self):
        return self._call("ntaps")

    def is_sparse(self):
        """True when FAST mode runs the kernel that uses the Hilbert structure of the taps"""
        return bool(self._call("is_sparse"))

    def taps(self):
        out = np.zeros(self.ntaps(), dtype=np.float32)
        n = self._call("taps", _ptr(out), len(out))
        return out[:n]

    def _input(self, noutput_items, a):
        x = np.ascontiguousarray(a, dtype=np.float32)
        need = noutput_items + self.history() - 1
        if len(x) < need:
            raise ValueError("work needs %d input items, got %d" % (need, len(x)))
        return x


class hilbert_fc(_analytic):
    """gr.hilbert_fc(ntaps): real stream -> analytic signal; history ntaps | 1"""
    _name = "hilbert_fc"

    def __init__(self, ntaps, device=0):
        _Block.__init__(self)
        if int(ntaps) < 0:
            raise GrhipError(-1, "negative ntaps %d" % int(ntaps))
        self._create(int(ntaps), int(device))

    def work(self, noutput_items, input_items):
        x = self._input(noutput_items, input_items)
        out = np.zeros(noutput_items, dtype=np.complex64)
        n = self._call("work", int(noutput_items), _ptr(x), _ptr(out))
        return out[:n]


class filter_delay_fc(_analytic):
    """gr.filter_delay_fc(taps): out = (in0 delayed by ntaps/2, taps * in1); one input: in1 = in0"""
    _name = "filter_delay_fc"

    def __init__(self, taps, device=0):
        _Block.__init__(self)
        t = np.ascontiguousarray(taps, dtype=np.float32)
        self._create(_ptr(t) if len(t) else None, len(t), int(device))

    def work(self, noutput_items, input_items, input_items1=None):
        x0 = self._input(noutput_items, input_items)
        x1 = None if input_items1 is None else self._input(noutput_items, input_items1)
        out = np.zeros(noutput_items, dtype=np.complex64)
        n = self._call("work", int(noutput_items), _ptr(x0), None if x1 is None else _ptr(x1), _ptr(out))
        return out[:n]

    def work_device(self, noutput_items, d_in0, d_in1, d_out, stream=None):
        return self._call("work_device", int(noutput_items), _devptr(d_in0), _devptr(d_in1), _devptr(d_out),
                          _stream(stream))


class goertzel_fc(_Block):
    """gr.goertzel_fc(rate, len, freq): one DFT bin per block of len floats (a sync decimator by len)"""
    _name = "goertzel_fc"

    def __init__(self, rate, len, freq, device=0):
        _Block.__init__(self)
        self._create(int(rate), int(len), float(freq), int(device))

    def set_freq(self, freq):
        self._call("set_freq", float(freq))

    def set_rate(self, rate):
        self._call("set_rate", int(rate))

    def history(self):
        return 1

    def decimation(self):
        return self._call("decimation")

    def work(self, noutput_items, input_items):
        x = np.ascontiguousarray(input_items, dtype=np.float32)
        if len(x) < noutput_items * self.decimation():
            raise ValueError("not enough input")
        out = np.zeros(noutput_items, dtype=np.complex64)
        n = self._call("work", int(noutput_items), _ptr(x), _ptr(out))
        return out[:n]


# ----------------------------------------------------------------------------
# gr.dc_blocker_ff / _cc, gr.moving_average_XX, gr.integrate_XX  (filter/gr_dc_blocker_ff.i, gengen/gr_moving_average_XX.i.t,
# gengen/gr_integrate_XX.i.t)
# ----------------------------------------------------------------------------
_RUNSUM_DTYPE = {"ff": np.float32, "cc": np.complex64, "ss": np.int16, "ii": np.int32}


class _runsum(_Block):
    _dtype = property(lambda self: _RUNSUM_DTYPE[self._name[-2:]])

    def _work(self, n, x, nout):
        out = np.zeros(nout, dtype=self._dtype)
        r = self._call("work", int(n), _ptr(x), _ptr(out))
        return out, r


class _dc_blocker(_stream_block):
    """gr.dc_blocker_XX(D=32, long_form=True): the input delayed by get_group_delay() minus 2 or 4 cascaded D-point
    moving averages of it.  The state lives in the block and carries across work calls; set_streams restarts the
    filter."""
    _in = _out = _runsum._dtype

    def __init__(self, D=32, long_form=True, device=0):
        _Block.__init__(self)
        self._create(int(D), 1 if long_form else 0, int(device))

    def get_group_delay(self):
        return self._call("group_delay")

    def decimation(self):
        return 1

    def work(self, noutput_items, input_items):
        return self._stream_work(input_items, noutput_items)


class dc_blocker_ff(_dc_blocker):
    _name = "dc_blocker_ff"


class dc_blocker_cc(_dc_blocker):
    _name = "dc_blocker_cc"


class _moving_average(_runsum):
    """gr.moving_average_XX(length, scale, max_iter=4096): history length; work returns min(noutput_items, max_iter)
    outputs, as one reference work call; work_device stands for successive calls of max_iter outputs."""

    def _scale_args(self, scale):
        k = self._name[-2:]
        if k == "ff":
            return [float(scale)]
        if k == "cc":
            z = complex(scale)
            return [z.real, z.imag]
        return [int(scale)]

    def __init__(self, length, scale, max_iter=4096, device=0):
        _Block.__init__(self)
        self._create(int(length), *(self._scale_args(scale) + [int(max_iter), int(device)]))

    def set_length_and_scale(self, length, scale):
        self._call("set_length_and_scale", int(length), *self._scale_args(scale))

    def history(self):
        return self._call("history")

    def max_iter(self):
        return self._call("max_iter")

    def decimation(self):
        return 1

    def work(self, noutput_items, input_items):
        x = np.ascontiguousarray(input_items, dtype=self._dtype)
        need = min(noutput_items, self.max_iter()) + self.history() - 1
        if len(x) < need:
            raise ValueError("work needs %d input items, got %d" % (need, len(x)))
        out, r = self._work(noutput_items, x, max(noutput_items, 1))
        return out[:r]


class moving_average_ff(_moving_average):
    _name = "moving_average_ff"


class moving_average_cc(_moving_average):
    _name = "moving_average_cc"


class moving_average_ss(_moving_average):
    _name = "moving_average_ss"


class moving_average_ii(_moving_average):
    _name = "moving_average_ii"


class _integrate(_runsum):
    """gr.integrate_XX(decim): out[i] = sum of in[i decim .. i decim + decim - 1] (a sync decimator by decim)"""

    def __init__(self, decim, device=0):
        _Block.__init__(self)
        self._create(int(decim), int(device))

    def history(self):
        return 1

    def decimation(self):
        return self._call("decimation")

    def work(self, noutput_items, input_items):
        x = np.ascontiguousarray(input_items, dtype=self._dtype)
        if len(x) < noutput_items * self.decimation():
            raise ValueError("not enough input")
        out, r = self._work(noutput_items, x, noutput_items)
        return out[:r]


class integrate_ff(_integrate):
    _name = "integrate_ff"


class integrate_cc(_integrate):
    _name = "integrate_cc"


class integrate_ss(_integrate):
    _name = "integrate_ss"


class integrate_ii(_integrate):
    _name = "integrate_ii"


# ----------------------------------------------------------------------------
# gr.complex_to_mag_squared, gr.single_pole_iir_filter_ff, gr.nlog10_ff, gr.keep_one_in_n (general/gr_complex_to_xxx.i,
# filter/gr_single_pole_iir_filter_ff.i, general/gr_nlog10_ff.i, general/gr_keep_one_in_n.i)
# ----------------------------------------------------------------------------
class _spectrum(_stream_block):
    _in = _out = np.float32

    def __init__(self, vlen):
        _Block.__init__(self)
        self._per_in = self._per_out = int(vlen)

    def work(self, noutput_items, input_items):
        """items are vectors of vlen; input_items holds streams x noutput_items of them"""
        return self._stream_work(input_items, noutput_items)


class complex_to_mag_squared(_spectrum):
    """gr.complex_to_mag_squared(vlen=1): re * re + im * im, unfused"""
    _name = "complex_to_mag_squared"
    _in = np.complex64

    def __init__(self, vlen=1, device=0):
        _spectrum.__init__(self, vlen)
        self._create(int(vlen), int(device))


class complex_to_mag(_spectrum):
    """gr.complex_to_mag(vlen=1): (float)sqrt((double)re * re + (double)im * im), the same in every mode"""
    _name = "complex_to_mag"
    _in = np.complex64

    def __init__(self, vlen=1, device=0):
        _spectrum.__init__(self, vlen)
        self._create(int(vlen), int(device))


class single_pole_iir_filter_ff(_spectrum):
    """gr.single_pole_iir_filter_ff(alpha, vlen=1): y = alpha x + (1 - alpha) y_prev per element, taps in double, state
    in float; the state carries across work calls and set_taps keeps it"""
    _name = "single_pole_iir_filter_ff"

    def __init__(self, alpha, vlen=1, device=0):
        _spectrum.__init__(self, vlen)
        self._create(float(alpha), int(vlen), int(device))

    def set_taps(self, alpha):
        self._call("set_taps", float(alpha))

    @staticmethod
    def chunk():
        """items per chunk of the FAST mode's cut of the item axis"""
        return lib().grhip_single_pole_iir_filter_ff_chunk()


class nlog10_ff(_spectrum):
    """gr.nlog10_ff(n=1, vlen=1, k=0): n * log10(max(x, 1e-18)) + k"""
    _name = "nlog10_ff"

    def __init__(self, n=1, vlen=1, k=0, device=0):
        _spectrum.__init__(self, vlen)
        self._create(float(n), int(vlen), float(k), int(device))


class _squelch_streams(_Block):
    """what every squelch block shares: work(x) takes streams x n_in items back to back and returns every stream's
    produced items (one array for one stream, a list otherwise); the detector and the ramp machine carry across calls.
    set_streams restarts every stream from the reference's initial state."""
    _in = np.complex64

    def unmuted(self, stream=0):
        return bool(self._call("unmuted", int(stream)))

    def work_into(self, n_in, input_items, out):
        """the raw call: `out` (streams x n_in items, C-contiguous) is written up to every stream's count; returns the counts"""
        x = np.ascontiguousarray(input_items, dtype=self._in).reshape(-1)
        if len(x) < n_in * self._streams or out.size < n_in * self._streams or out.dtype != self._in:
            raise ValueError("work needs %d items in and room for as many out" % (n_in * self._streams))
        produced = np.zeros(self._streams, dtype=np.int32)
        self._call("work", int(n_in), _ptr(x), _ptr(out), _ptr(produced))
        if n_in == 0:
            produced[:] = 0
        return produced

    def work(self, input_items, n_in=None):
        x, n_in = self._work_in(input_items, n_in)
        out = np.zeros(max(n_in * self._streams, 1), dtype=self._in)
        p = self.work_into(n_in, x, out)
        res = [out[s * n_in:s * n_in + int(p[s])] for s in range(self._streams)]
        return res[0] if self._streams == 1 else res

    def work_device(self, n_in, d_in, d_out, d_produced, stream=None):
        """device buffers; d_produced holds streams int32 counts; does not synchronise"""
        return self._call("work_device", int(n_in), _devptr(d_in), _devptr(d_out), _devptr(d_produced), _stream(stream))


class _ramp_gate(object):
    """ramp() / gate() and their setters (general/gr_squelch_base_cc.h:45-48)"""

    def ramp(self):
        return self._call("ramp")

    def set_ramp(self, ramp):
        self._call("set_ramp", int(ramp))

    def gate(self):
        return bool(self._call("gate"))

    def set_gate(self, gate):
        self._call("set_gate", int(bool(gate)))


class _squelch(_squelch_streams):
    """gr.pwr_squelch_cc / _ff and gr.simple_squelch_cc (general/gr_pwr_squelch_cc.i, gr_pwr_squelch_ff.i,
    gr_simple_squelch_cc.i): the power detector's accessors"""

    def threshold(self):
        return self._fn("threshold")(self._h)

    def set_threshold(self, db):
        self._call("set_threshold", float(db))

    def set_alpha(self, alpha):
        self._call("set_alpha", float(alpha))

    def state(self, stream=0):
        """(state, ramped, envelope, detector output) of one stream; state 0 muted, 1 attack, 2 unmuted, 3 decay"""
        st, r, e, y = C.c_int(0), C.c_int(0), C.c_double(0), C.c_double(0)
        self._call("state", int(stream), C.byref(st), C.byref(r), C.byref(e), C.byref(y))
        return st.value, r.value, e.value, y.value

    @staticmethod
    def squelch_range():
        return [-50.0, 50.0, 1.0]

    @staticmethod
    def chunk():
        """samples per chunk of the FAST detector's cut of the item axis"""
        return lib().grhip_pwr_squelch_chunk()


class _pwr_squelch(_squelch, _ramp_gate):
    def __init__(self, db, alpha=0.0001, ramp=0, gate=False, device=0):
        _Block.__init__(self)
        self._create(float(db), float(alpha), int(ramp), int(bool(gate)), int(device))


class pwr_squelch_cc(_pwr_squelch):
    """gr.pwr_squelch_cc(db, alpha=0.0001, ramp=0, gate=False)"""
    _name = "pwr_squelch_cc"


class pwr_squelch_ff(_pwr_squelch):
    """gr.pwr_squelch_ff(db, alpha=0.0001, ramp=0, gate=False)"""
    _name = "pwr_squelch_ff"
    _in = np.float32


class simple_squelch_cc(_squelch):
    """gr.simple_squelch_cc(threshold_db, alpha): out = in where the detector is at or above the threshold, else 0"""
    _name = "simple_squelch_cc"

    def __init__(self, threshold_db, alpha=0.0001, device=0):
        _Block.__init__(self)
        self._create(float(threshold_db), float(alpha), int(device))


class ctcss_squelch_ff(_squelch_streams, _ramp_gate):
    """gr.ctcss_squelch_ff(rate, freq, level=0.01, len=0, ramp=0, gate=False) (general/gr_ctcss_squelch_ff.i): mutes
    unless the tone at freq stands above level and above its two guard tones, decided once per len samples (len 0:
    rate / 10).  work() as the power squelch blocks; blocks of len samples run across calls."""
    _name = "ctcss_squelch_ff"
    _in = np.float32

    def __init__(self, rate, freq, level=0.01, len=0, ramp=0, gate=False, device=0):
        _Block.__init__(self)
        self._create(int(rate), float(freq), float(level), int(len), int(ramp), int(bool(gate)), int(device))

    def level(self):
        return self._fn("level")(self._h)

    def set_level(self, level):
        self._call("set_level", float(level))

    def len(self):
        return self._call("len")

    @staticmethod
    def squelch_range():
        r = (C.c_float * 3)()
        _check(lib().grhip_ctcss_squelch_ff_squelch_range(r))
        return [r[0], r[1], r[2]]

    def state(self, stream=0):
        """(state, ramped, envelope, d_mute, samples of the unfinished block) of one stream"""
        st, r, e, m, p = C.c_int(0), C.c_int(0), C.c_double(0), C.c_int(0), C.c_int(0)
        self._call("state", int(stream), C.byref(st), C.byref(r), C.byref(e), C.byref(m), C.byref(p))
        return st.value, r.value, e.value, bool(m.value), p.value

    def tones(self):
        """(left guard, tone, right guard) in Hz, as float32"""
        v = [C.c_float(0), C.c_float(0), C.c_float(0)]
        self._call("tones", C.byref(v[0]), C.byref(v[1]), C.byref(v[2]))
        return tuple(np.float32(x.value) for x in v)

    def last_magnitudes(self, n_blocks, stream=0):
        """|l|, |c|, |r| of the blocks the last work call completed, [blocks][3] float32 (for tests)"""
        out = np.zeros((max(int(n_blocks), 1), 3), dtype=np.float32)
        got = self._call("last_magnitudes", int(stream), _ptr(out), int(n_blocks))
        return out[:got]


class _agc(_stream_block):
    """what the four gain loops share: work(x) takes streams x n_in items back to back and returns as many; every
    stream's gain carries across calls.  The setters act at once (they hold from the next work call), as the
    reference's do; set_gain sets every stream's gain, and set_streams sets it to the constructor's.  work_device
    does not synchronise.  The float getters return the value itself, not a status."""
    _in = _out = np.complex64

    def reference(self):
        return self._fn("reference")(self._h)

    def set_reference(self, reference):
        self._call("set_reference", float(reference))

    def max_gain(self):
        return self._fn("max_gain")(self._h)

    def set_max_gain(self, max_gain):
        self._call("set_max_gain", float(max_gain))

    def gain(self, stream=0):
        return np.float32(self._stream_value("gain", C.c_float, stream))

    def set_gain(self, gain):
        self._call("set_gain", float(gain))

    def work(self, input_items, n_in=None):
        return self._stream_work(input_items, n_in)

    @staticmethod
    def chunk():
        """items per chunk of the chunked form of agc_cc / agc_ff"""
        return lib().grhip_agc_chunk()


class _agc1(_agc):
    def __init__(self, rate=1e-4, reference=1.0, gain=1.0, max_gain=0.0, device=0):
        _Block.__init__(self)
        self._create(float(rate), float(reference), float(gain), float(max_gain), int(device))

    def rate(self):
        return self._fn("rate")(self._h)

    def set_rate(self, rate):
        self._call("set_rate", float(rate))


class _agc2(_agc):
    def __init__(self, attack_rate=1e-1, decay_rate=1e-2, reference=1.0, gain=1.0, max_gain=0.0, device=0):
        _Block.__init__(self)
        self._create(float(attack_rate), float(decay_rate), float(reference), float(gain), float(max_gain), int(device))

    def attack_rate(self):
        return self._fn("attack_rate")(self._h)

    def set_attack_rate(self, rate):
        self._call("set_attack_rate", float(rate))

    def decay_rate(self):
        return self._fn("decay_rate")(self._h)

    def set_decay_rate(self, rate):
        self._call("set_decay_rate", float(rate))


class agc_cc(_agc1):
    """gr.agc_cc(rate=1e-4, reference=1.0, gain=1.0, max_gain=0.0) (general/gr_agc_cc.i): out = in * gain, then
    gain += rate * (reference - |out|), clamped to max_gain where that is positive.  MODE_GENERIC is the reference's
    float recurrence bit for bit; every other mode runs calls of more than chunk() items in chunks."""
    _name = "agc_cc"


class agc_ff(_agc1):
    """gr.agc_ff(rate=1e-4, reference=1.0, gain=1.0, max_gain=0.0) (general/gr_agc_ff.i): agc_cc on floats"""
    _name = "agc_ff"
    _in = _out = np.float32


class agc2_cc(_agc2):
    """gr.agc2_cc(attack_rate=1e-1, decay_rate=1e-2, reference=1.0, gain=1.0, max_gain=0.0) (general/gr_agc2_cc.i):
    the rate is attack_rate where |out| - reference exceeds the gain and decay_rate otherwise; a negative gain
    becomes 10e-5.  Every mode is the reference's recurrence bit for bit."""
    _name = "agc2_cc"


class agc2_ff(_agc2):
    """gr.agc2_ff(attack_rate=1e-1, decay_rate=1e-2, reference=1.0, gain=1.0, max_gain=0.0) (general/gr_agc2_ff.i):
    agc2_cc on floats, with the rate test on the magnitude of |out| - reference as the reference has it"""
    _name = "agc2_ff"
    _in = _out = np.float32


# ----------------------------------------------------------------------------
# digital.costas_loop_cc, gr.pll_freqdet_cf, gr.pll_refout_cc, gr.pll_carriertracking_cc  (gr-digital/swig/
# digital_costas_loop_cc.i, general/gr_pll_*.i, general/gri_control_loop.i)
# ----------------------------------------------------------------------------
class _control_loop(_stream_block):
    """what the four carrier loops share: gri_control_loop's setters and getters under their own names, and
    work(x), which takes streams x n_in complex items back to back.  Phase and frequency are per stream and carry
    across calls; a setter acts at once on every stream.  A value the reference refuses with std::out_of_range
    raises GrhipError (code -1).  work_device does not synchronise."""
    _in = _out = np.complex64

    def set_loop_bandwidth(self, bw):
        self._call("set_loop_bandwidth", float(bw))

    def set_damping_factor(self, df):
        self._call("set_damping_factor", float(df))

    def set_alpha(self, alpha):
        self._call("set_alpha", float(alpha))

    def set_beta(self, beta):
        self._call("set_beta", float(beta))

    def set_frequency(self, freq):
        self._call("set_frequency", float(freq))

    def set_phase(self, phase):
        self._call("set_phase", float(phase))

    def get_loop_bandwidth(self):
        return self._fn("get_loop_bandwidth")(self._h)

    def get_damping_factor(self):
        return self._fn("get_damping_factor")(self._h)

    def get_alpha(self):
        return self._fn("get_alpha")(self._h)

    def get_beta(self):
        return self._fn("get_beta")(self._h)

    def get_frequency(self, stream=0):
        return np.float32(self._stream_value("get_frequency", C.c_float, stream))

    def get_phase(self, stream=0):
        return np.float32(self._stream_value("get_phase", C.c_float, stream))

    def work(self, input_items, n_in=None):
        return self._stream_work(input_items, n_in)


class _pll(_control_loop):
    def __init__(self, loop_bw, max_freq, min_freq, device=0):
        _Block.__init__(self)
        self._create(float(loop_bw), float(max_freq), float(min_freq), int(device))


class pll_freqdet_cf(_pll):
    """gr.pll_freqdet_cf(loop_bw, max_freq, min_freq) (general/gr_pll_freqdet_cf.i): the loop's frequency in front of
    every sample, in rad/sample.  Bit for bit the reference in every mode."""
    _name = "pll_freqdet_cf"
    _out = np.float32


class pll_refout_cc(_pll):
    """gr.pll_refout_cc(loop_bw, max_freq, min_freq) (general/gr_pll_refout_cc.i): (cos, sin) of the loop's phase in
    front of every sample.  The state is the reference's bit for bit, the outputs within one float ulp."""
    _name = "pll_refout_cc"


class pll_carriertracking_cc(_pll):
    """gr.pll_carriertracking_cc(loop_bw, max_freq, min_freq) (general/gr_pll_carriertracking_cc.i): the input mixed
    down by the loop's phase, a lock signal, and an optional squelch on it."""
    _name = "pll_carriertracking_cc"

    def lock_detector(self, stream=0):
        return bool(self._stream_value("lock_detector", C.c_int, stream))

    def locksig(self, stream=0):
        return np.float32(self._stream_value("locksig", C.c_float, stream))

    def squelch_enable(self, enable):
        self._call("squelch_enable", int(bool(enable)))
        return bool(enable)

    def set_lock_threshold(self, threshold):
        self._call("set_lock_threshold", float(threshold))
        return float(threshold)


class costas_loop_cc(_control_loop):
    """digital.costas_loop_cc(loop_bw, order) (gr-digital/swig/digital_costas_loop_cc.i), order 2, 4 or 8.
    work(x) returns the derotated samples; work(x, freq=True) returns (out, freq) with the loop's frequency behind
    every sample.  MODE_GENERIC runs the float-rounded double sine and cosine in the NCO, every other mode a float
    polynomial; neither is the reference's sincosf to the bit (include/grhip.h)."""
    _name = "costas_loop_cc"

    def __init__(self, loop_bw, order, device=0):
        _Block.__init__(self)
        self._create(float(loop_bw), int(order), int(device))

    def work(self, input_items, n_in=None, freq=False):
        return self._stream_work(input_items, n_in, [np.float32], freq)

    def work_device(self, n, d_in, d_out, d_freq_out=None, stream=None):
        return self._call("work_device", int(n), _devptr(d_in), _devptr(d_out), _devptr(d_freq_out), _stream(stream))


class fll_band_edge_cc(_control_loop):
    """digital.fll_band_edge_cc(samps_per_sym, rolloff, filter_size, bandwidth) (gr-digital/swig/
    digital_fll_band_edge_cc.i): the band-edge frequency-lock loop.  work(x) returns the derotated samples, delayed
    by 2 * filter_size - 1 items; work(x, aux=True) returns (out, frq, phs, err) with the loop's frequency, phase and
    error behind every step.  The handle takes new items only and keeps what it needs of the past per stream, so the
    result depends on the concatenated input alone (include/grhip.h).  MODE_GENERIC is bit for bit the restatement in
    tests/fll_ref.py; every other mode runs the float NCO, fused products and tree-order sums."""
    _name = "fll_band_edge_cc"

    def __init__(self, samps_per_sym, rolloff, filter_size, bandwidth, device=0):
        _Block.__init__(self)
        self._create(float(samps_per_sym), float(rolloff), int(filter_size), float(bandwidth), int(device))

    def history(self):
        return self.get_filter_size() + 1           # digital_fll_band_edge_cc.cc:187

    def set_samples_per_symbol(self, sps):
        self._call("set_samples_per_symbol", float(sps))

    def set_rolloff(self, rolloff):
        self._call("set_rolloff", float(rolloff))

    def set_filter_size(self, filter_size):
        """a new filter size also zeroes every stream's two histories (phase and frequency stay)"""
        self._call("set_filter_size", int(filter_size))

    def get_samples_per_symbol(self):
        return self._fn("get_samples_per_symbol")(self._h)

    def get_rolloff(self):
        return self._fn("get_rolloff")(self._h)

    def get_filter_size(self):
        return self._call("get_filter_size")

    def work(self, input_items, n_in=None, aux=False):
        return self._stream_work(input_items, n_in, [np.float32] * 3, aux)

    def work_device(self, n, d_in, d_out, d_frq=None, d_phs=None, d_err=None, stream=None):
        return self._call("work_device", int(n), _devptr(d_in), _devptr(d_out), _devptr(d_frq), _devptr(d_phs), _devptr(d_err),
                          _stream(stream))


def fll_band_edge_taps(samps_per_sym, rolloff, filter_size):
    """(lower, upper): digital_fll_band_edge_cc::design_filter's two tap sets as the reference stores them (reversed).
    Host arithmetic only, no device needed.  A refused design is a GrhipError."""
    n = max(int(filter_size), 1)
    lower, upper = np.zeros(min(n, 1024), dtype=np.complex64), np.zeros(min(n, 1024), dtype=np.complex64)
    _check(lib().grhip_fll_band_edge_taps(float(samps_per_sym), float(rolloff), int(filter_size), _ptr(lower), _ptr(upper)))
    return lower, upper


def firdes_root_raised_cosine(gain, sampling_freq, symbol_rate, alpha, ntaps):
    """gr.firdes.root_raised_cosine(gain, sampling_freq, symbol_rate, alpha, ntaps): host arithmetic only, no device
    needed.  A failed argument check is a GrhipError."""
    args = (float(gain), float(sampling_freq), float(symbol_rate), float(alpha), int(ntaps))
    n = C.c_size_t(0)
    rc = lib().grhip_firdes_root_raised_cosine(*(args + (C.c_void_p(0), 0, C.byref(n))))
    if rc != -2:                                    # GRHIP_ERANGE: the size query's answer
        _check(rc)
    out = np.zeros(max(n.value, 1), dtype=np.float32)
    _check(lib().grhip_firdes_root_raised_cosine(*(args + (_ptr(out), n.value, C.byref(n)))))
    return out[:n.value]


class pfb_clock_sync_ccf(_Block):
    """gr.pfb_clock_sync_ccf(sps, loop_bw, taps, filter_size=32, init_phase=0, max_rate_deviation=1.5, osps=1)
    (filter/gr_pfb_clock_sync_ccf.i): polyphase timing recovery.  work(x) returns one array of symbols per stream (a
    single array for one stream); work(x, aux=True) returns (out, err, rate, k) likewise.  The handle takes new items
    only and keeps what it needs of the past per stream, so the result depends on the concatenated input alone
    (include/grhip.h).  MODE_GENERIC is bit for bit the restatement in tests/pfb_clock_sync_ref.py and through it the
    reference; every other mode runs the same scalar loop with fused products and tree-order sums."""
    _name = "pfb_clock_sync_ccf"
    _in = np.complex64

    def __init__(self, sps, loop_bw, taps, filter_size=32, init_phase=0.0, max_rate_deviation=1.5, osps=1, device=0):
        _Block.__init__(self)
        t = np.ascontiguousarray(taps, dtype=np.float32)
        self._create(float(sps), float(loop_bw), _ptr(t), len(t), int(filter_size), float(init_phase), float(max_rate_deviation),
                     int(osps), int(device))

    def set_loop_bandwidth(self, bw):
        self._call("set_loop_bandwidth", float(bw))

    def set_damping_factor(self, df):
        self._call("set_damping_factor", float(df))

    def set_alpha(self, alpha):
        self._call("set_alpha", float(alpha))

    def set_beta(self, beta):
        self._call("set_beta", float(beta))

    def set_max_rate_deviation(self, m):
        self._call("set_max_rate_deviation", float(m))

    def get_loop_bandwidth(self):
        return self._fn("get_loop_bandwidth")(self._h)

    def get_damping_factor(self):
        return self._fn("get_damping_factor")(self._h)

    def get_alpha(self):
        return self._fn("get_alpha")(self._h)

    def get_beta(self):
        return self._fn("get_beta")(self._h)

    def get_max_rate_deviation(self):
        return self._fn("get_max_rate_deviation")(self._h)

    def get_clock_rate(self, stream=0):
        return np.float32(self._stream_value("get_clock_rate", C.c_float, stream))

    def k(self, stream=0):
        return np.float32(self._stream_value("k", C.c_float, stream))

    def error(self, stream=0):
        return np.float32(self._stream_value("error", C.c_float, stream))

    def slips(self, stream=0):
        return self._stream_value("slips", C.c_int, stream)

    def position(self, stream=0):
        """the index into xz (tpf + floor(sps) - 1 zeros, then the stream) at which the next symbol starts"""
        return self._stream_value("position", C.c_longlong, stream)

    def _bank(self, name):
        nf, tpf = C.c_int(0), C.c_int(0)
        rc = self._fn(name)(self._h, C.c_void_p(0), 0, C.byref(nf), C.byref(tpf))
        if rc != -2:                                    # GRHIP_ERANGE: the size query's answer
            _check(rc)
        b = np.zeros((nf.value, tpf.value), dtype=np.float32)
        self._call(name, _ptr(b), b.size, C.byref(nf), C.byref(tpf))
        return b

    def get_taps(self):
        return self._bank("get_taps")

    def get_diff_taps(self):
        return self._bank("get_diff_taps")

    def max_produced(self, n_in):
        return self._call("max_produced", int(n_in))

    def work(self, input_items, n_in=None, aux=False):
        x, n_in = self._work_in(input_items, n_in)
        cap = self.max_produced(n_in)
        S = self._streams
        out = np.zeros((S, cap), dtype=np.complex64)
        f = [np.zeros((S, cap), dtype=np.float32) for _ in range(3)] if aux else []
        prod = np.zeros(S, dtype=np.int32)
        null = C.c_void_p(0)
        if len(x) == 0:
            x = np.zeros(1, np.complex64)
        self._call("work", int(n_in), _ptr(x), cap, _ptr(out), *([_ptr(a) for a in f] if aux else [null, null, null]) + [_ptr(prod)])
        rows = [tuple(a[s, :prod[s]].copy() for a in [out] + f) if aux else out[s, :prod[s]].copy() for s in range(S)]
        return rows[0] if S == 1 else rows

    def work_device(self, n, d_in, out_cap, d_out, d_produced, d_err=None, d_rate=None, d_k=None, stream=None):
        return self._call("work_device", int(n), _devptr(d_in), int(out_cap), _devptr(d_out), _devptr(d_err), _devptr(d_rate),
                          _devptr(d_k), _devptr(d_produced), _stream(stream))


def pfb_clock_sync_taps(taps, filter_size):
    """(bank, diff_bank): gr_pfb_clock_sync_ccf's two polyphase banks as get_taps() and get_diff_taps() return them,
    [filter_size][taps per arm].  Host arithmetic only, no device needed.  A refused prototype is a GrhipError."""
    t = np.ascontiguousarray(taps, dtype=np.float32)
    tpf = C.c_int(0)
    _check(lib().grhip_pfb_clock_sync_taps(_ptr(t), len(t), int(filter_size), C.c_void_p(0), C.c_void_p(0), C.byref(tpf)))
    bank, dbank = np.zeros((int(filter_size), tpf.value), np.float32), np.zeros((int(filter_size), tpf.value), np.float32)
    _check(lib().grhip_pfb_clock_sync_taps(_ptr(t), len(t), int(filter_size), _ptr(bank), _ptr(dbank), C.byref(tpf)))
    return bank, dbank


# ----------------------------------------------------------------------------
# digital.constellation_* and the blocks behind timing recovery (gr-digital/swig/digital_constellation.i,
# digital_constellation_receiver_cb.i, digital_constellation_decoder_cb.i, general/gr_diff_decoder_bb.i, gr_map_bb.i,
# gr-digital/python/generic_mod_demod.py:296-313, psk.py, qam.py, utils/gray_code.py, utils/mod_codes.py)
# ----------------------------------------------------------------------------
def _points(points):
    p = np.ascontiguousarray(points, dtype=np.complex64).reshape(-1)
    return p, (_ptr(p) if len(p) else C.c_void_p(0)), len(p)


def _code(code):
    c = np.ascontiguousarray(code, dtype=np.uint32).reshape(-1)
    return c, (_ptr(c) if len(c) else C.c_void_p(0)), len(c)


class constellation(object):
    """a digital_constellation: a host object, no device needed.  Made by constellation_bpsk() ... constellation_rect()."""

    def __init__(self, kind, *args):
        self._h = C.c_void_p(0)
        _check(getattr(lib(), "grhip_constellation_create_" + kind)(C.byref(self._h), *args))

    def __del__(self):
        try:
            if self._h:
                lib().grhip_constellation_destroy(self._h)
                self._h = C.c_void_p(0)
        except Exception:
            pass

    def _int(self, name):
        return _check(getattr(lib(), "grhip_constellation_" + name)(self._h))

    def _array(self, name, dtype, width=1):
        n = _check(getattr(lib(), "grhip_constellation_" + name)(self._h, C.c_void_p(0), 0))
        a = np.zeros(max(n * width, 1), dtype)
        _check(getattr(lib(), "grhip_constellation_" + name)(self._h, _ptr(a), n))
        return a[:n * width]

    def base(self):
        return self

    def arity(self):
        return self._int("arity")

    def dimensionality(self):
        return self._int("dimensionality")

    def rotational_symmetry(self):
        return self._int("rotational_symmetry")

    def bits_per_symbol(self):
        return self._int("bits_per_symbol")

    def apply_pre_diff_code(self):
        return bool(self._int("apply_pre_diff_code"))

    def points(self):
        return self._array("points", np.float32, 2).view(np.complex64)

    def pre_diff_code(self):
        return [int(v) for v in self._array("pre_diff_code", np.uint32)]

    def sector_values(self):
        return self._array("sector_values", np.uint32)

    def decision_maker(self, sample):
        """the symbols of items of dimensionality() samples each (one item, or an array of them)"""
        return self.decision_maker_pe(sample, errors=False)

    def decision_maker_pe(self, sample, errors=True):
        x = np.ascontiguousarray(sample, dtype=np.complex64).reshape(-1, self.dimensionality())
        idx, pe = np.zeros(len(x), np.uint32), np.zeros(len(x), np.float32)
        k, e = C.c_uint(0), C.c_float(0)
        L = lib()
        for i in range(len(x)):
            if errors:
                _check(L.grhip_constellation_decision_maker_pe(self._h, x[i].ctypes.data, C.byref(k), C.byref(e)))
                pe[i] = e.value
            else:
                _check(L.grhip_constellation_decision_maker(self._h, x[i].ctypes.data, C.byref(k)))
            idx[i] = k.value
        scalar = np.ndim(sample) == 0 or (self.dimensionality() > 1 and np.ndim(sample) == 1 and len(x) == 1)
        if not errors:
            return int(idx[0]) if scalar else idx
        return (int(idx[0]), np.float32(pe[0])) if scalar else (idx, pe)


def constellation_bpsk():
    return constellation("bpsk")


def constellation_qpsk():
    return constellation("qpsk")


def constellation_dqpsk():
    return constellation("dqpsk")


def constellation_8psk():
    return constellation("8psk")


def constellation_calcdist(points, pre_diff_code, rotational_symmetry, dimensionality):
    p, pp, n = _points(points)
    c, pc, m = _code(pre_diff_code)
    return constellation("calcdist", pp, n, pc, m, int(rotational_symmetry), int(dimensionality))


def constellation_psk(points, pre_diff_code, n_sectors):
    p, pp, n = _points(points)
    c, pc, m = _code(pre_diff_code)
    return constellation("psk", pp, n, pc, m, int(n_sectors))


def constellation_rect(points, pre_diff_code, rotational_symmetry, real_sectors, imag_sectors, width_real_sectors,
                       width_imag_sectors):
    p, pp, n = _points(points)
    c, pc, m = _code(pre_diff_code)
    return constellation("rect", pp, n, pc, m, int(rotational_symmetry), int(real_sectors), int(imag_sectors),
                         float(width_real_sectors), float(width_imag_sectors))


def gray_code(length):
    """utils/gray_code.py: the first `length` Gray code words"""
    gcs, lp2, np2, i = [0, 1], 2, 4, 2
    while len(gcs) < length:
        gcs.append(i + i // 2 if i == lp2 else gcs[2 * lp2 - 1 - i] + lp2)
        i += 1
        if i == np2:
            lp2, np2 = i, i * 2
    return gcs[:length]


def invert_code(code):
    """utils/mod_codes.py invert_code"""
    return [a for (b, a) in sorted((b, a) for (a, b) in enumerate(code))]


def psk_constellation(m=4, mod_code="gray"):
    """psk.py psk_constellation: m points on the unit circle, m sectors; mod_code 'gray' or 'none'"""
    k = math.log(m) / math.log(2.0)
    if k != int(k):
        raise ValueError("Number of constellation points must be a power of two.")
    if mod_code not in ("gray", "none"):
        raise ValueError("That modulation code is not implemented for this constellation.")
    points = [complex(np.exp(2 * math.pi * 1j * i / m)) for i in range(m)]
    return constellation_psk(points, gray_code(m) if mod_code == "gray" else [], m)


def qam_constellation(constellation_points=16, differential=True, mod_code="none"):
    """qam.py qam_constellation: a square grid decided by constellation_rect; mod_code 'gray' or 'none'"""
    if mod_code not in ("gray", "none"):
        raise ValueError("Mod code is not implemented for QAM")
    m, gray = int(constellation_points), mod_code == "gray"
    k = int(math.log(m) / math.log(2.0))
    if m < 4 or 4 ** (k // 2) != m:
        raise ValueError("m must be a power of 4 integer.")

    def bits(x, n, w):
        return (x >> n) % (2 ** w)
    if differential:        # make_differential_constellation: the quadrant bits differential, the rest Gray or plain
        side = int(pow(m, 0.5) / 2)
        i_gcs = dict((v, key) for key, v in enumerate(gray_code(side))) if gray else dict((i, i) for i in range(side))
        step = 1 / (side - 0.5)
        g = [(i_gcs[gc] + 0.5) * step for gc in range(side)]
        quad = (lambda x, y: complex(g[x], g[y]), lambda x, y: complex(-g[y], g[x]), lambda x, y: complex(-g[x], -g[y]),
                lambda x, y: complex(g[y], -g[x]))
        h = (k - 2) // 2
        points = [quad[bits(i, k - 2, 2)](bits(i, h, h), bits(i, 0, h)) for i in range(m)]
    else:                   # make_non_differential_constellation
        side = int(pow(m, 0.5))
        i_gcs = invert_code(gray_code(side)) if gray else list(range(side))
        step = 2.0 / (side - 1)
        g = [-1 + i_gcs[gc] * step for gc in range(side)]
        points = [complex(g[bits(i, k // 2, k // 2)], g[bits(i, 0, k // 2)]) for i in range(m)]
    side = int(math.sqrt(m))
    width = 2.0 / (side - 1)
    return constellation_rect(points, [], 4, side, side, width, width)


class _byte_block(_stream_block):
    """bytes in and bytes out, unless the block says otherwise"""
    _in = _out = np.uint8


class constellation_decoder_cb(_byte_block):
    """digital.constellation_decoder_cb(constellation): one symbol byte per dimensionality() complex items, the
    constellation's decision_maker byte for byte"""
    _name = "constellation_decoder_cb"
    _in = np.complex64

    def __init__(self, constellation, device=0):
        _Block.__init__(self)
        self._per_in = constellation.dimensionality()
        self._create(constellation._h, int(device))


class diff_decoder_bb(_byte_block):
    """gr.diff_decoder_bb(modulus): (in[i] - in[i-1]) % modulus with the reference's int-to-unsigned conversion; the
    last byte of a call is kept per stream (0 at the start)"""
    _name = "diff_decoder_bb"

    def __init__(self, modulus, device=0):
        _Block.__init__(self)
        self._create(int(modulus), int(device))

    def history(self):
        return 2


class map_bb(_byte_block):
    """gr.map_bb(map): out = map[in], the identity behind the entries given"""
    _name = "map_bb"

    def __init__(self, map, device=0):
        _Block.__init__(self)
        m = np.ascontiguousarray(map, dtype=np.int32).reshape(-1)
        self._create(_ptr(m) if len(m) else C.c_void_p(0), len(m), int(device))


class constellation_receiver_cb(_control_loop):
    """digital.constellation_receiver_cb(constellation, loop_bw, fmin, fmax): the decision-directed carrier loop.
    work(x) returns the symbols; work(x, floats=True) returns (symbols, error, phase, freq), phase and frequency after
    each sample's update.  form() says how decision and error are formed: 0 the reference's statements (MODE_GENERIC),
    1 cartesian (rect, calcdist), 2 on the sample's angle (bpsk, qpsk, dqpsk, 8psk, psk)."""
    _name = "constellation_receiver_cb"
    _out = np.uint8
    FORM_GENERIC, FORM_CARTESIAN, FORM_ANGLE = 0, 1, 2

    def __init__(self, constellation, loop_bw, fmin, fmax, device=0):
        _Block.__init__(self)
        self._create(constellation._h, float(loop_bw), float(fmin), float(fmax), int(device))

    def form(self):
        return self._call("form")

    def work(self, input_items, n_in=None, floats=False):
        return self._stream_work(input_items, n_in, [np.float32] * 3, floats)

    def work_device(self, n, d_in, d_symbols, d_error=None, d_phase=None, d_freq=None, stream=None):
        return self._call("work_device", int(n), _devptr(d_in), _devptr(d_symbols), _devptr(d_error), _devptr(d_phase),
                          _devptr(d_freq), _stream(stream))


class constellation_demod_cb(_control_loop):
    """generic_demod behind timing recovery (generic_mod_demod.py:296-313) as one block: constellation_receiver_cb ->
    diff_decoder_bb(arity) if differential -> map_bb(invert_code(pre_diff_code)) if gray_coded and the constellation
    applies one -> unpack_k_bits_bb(bits_per_symbol).  work(x): streams x n complex items in, n * bits_per_symbol()
    bytes out per stream.  engine() 1 (the default) stores the bits from the receiver's walk, 0 runs the blocks in a
    row; the bytes are the same."""
    _name = "constellation_demod_cb"
    _out = np.uint8

    def __init__(self, constellation, loop_bw, fmin, fmax, differential=True, gray_coded=True, device=0):
        _Block.__init__(self)
        self._create(constellation._h, float(loop_bw), float(fmin), float(fmax), int(bool(differential)), int(bool(gray_coded)),
                     int(device))

    def form(self):
        return self._call("form")

    def engine(self):
        return self._call("engine")

    def set_engine(self, engine):
        self._call("set_engine", int(engine))

    def bits_per_symbol(self):
        return self._call("bits_per_symbol")

    _per_out = property(bits_per_symbol)


# ----------------------------------------------------------------------------
# the blocks in front of generic_mod's pulse shaper (gengen/gr_packed_to_unpacked_XX.i.t, gr_unpacked_to_packed_XX.i.t,
# gr_chunks_to_symbols_XX.i.t, gengen/gr_endianness.h, general/gr_diff_encoder_bb.i,
# gr-digital/python/generic_mod_demod.py:114-150)
# ----------------------------------------------------------------------------
GR_MSB_FIRST = 0
GR_LSB_FIRST = 1


class _pack_block(_Block):
    """a gr_block that repacks bits: streams x ninput bytes back to back in, streams x noutput_items bytes out; the
    bit index it keeps between calls is one value for all streams"""
    _in = _out = np.uint8

    def __init__(self, bits_per_chunk, endianness=GR_MSB_FIRST, device=0):
        _Block.__init__(self)
        self._create(int(bits_per_chunk), int(endianness), int(device))

    def history(self):
        return 1

    def forecast(self, noutput_items):
        return self._call("forecast", int(noutput_items))

    def general_work(self, noutput_items, input_items, ninput_items=None):
        """returns (out, consumed); input_items holds streams x ninput_items bytes (all of it by default)"""
        x, ninput_items = self._work_in(input_items, ninput_items)
        (p_out,), (out,) = self._work_out(int(noutput_items))
        consumed = C.c_int(0)
        n = self._call("general_work", int(noutput_items), ninput_items, _ptr(x), p_out, C.byref(consumed))
        return out[:n * self._streams].copy(), consumed.value

    def general_work_device(self, noutput_items, ninput_items, d_in, d_out, stream=None):
        """returns (produced, consumed), known at once; the outputs are in d_out once `stream` has run"""
        consumed = C.c_int(0)
        n = self._call("general_work_device", int(noutput_items), int(ninput_items), _devptr(d_in), _devptr(d_out),
                       C.byref(consumed), _stream(stream))
        return n, consumed.value


class packed_to_unpacked_bb(_pack_block):
    """gr.packed_to_unpacked_bb(bits_per_chunk, endianness): chunk i is the bits_per_chunk bits from bit
    d_index + i * bits_per_chunk of the bytes, the first one its most significant (also for GR_LSB_FIRST, which takes
    a byte's bits from the bottom)"""
    _name = "packed_to_unpacked_bb"


class unpacked_to_packed_bb(_pack_block):
    """gr.unpacked_to_packed_bb(bits_per_chunk, endianness): the inverse; the low bits_per_chunk bits of the input
    bytes, laid end to end, in bytes"""
    _name = "unpacked_to_packed_bb"


class diff_encoder_bb(_byte_block):
    """gr.diff_encoder_bb(modulus): out[i] = (in[i] + out[i-1]) % modulus stored as a byte; the last output is kept
    per stream (0 at the start)"""
    _name = "diff_encoder_bb"

    def __init__(self, modulus, device=0):
        _Block.__init__(self)
        self._create(int(modulus), int(device))


class chunks_to_symbols_bc(_byte_block):
    """gr.chunks_to_symbols_bc(symbol_table, D=1): n bytes in, n * D complex items out per stream,
    symbol_table[in * D : in * D + D]; an index outside the table gives zeros"""
    _name = "chunks_to_symbols_bc"
    _out = np.complex64

    def __init__(self, symbol_table, D=1, device=0):
        _Block.__init__(self)
        t, pt, n = _points(symbol_table)            # t owns the memory until the call returns
        self._create(pt, n, int(D), int(device))

    def D(self):
        return self._call("D")

    _per_out = property(D)


class generic_mod(_Block):
    """digital.generic_mod (generic_mod_demod.py:76-157) as one block: packed_to_unpacked_bb(bits_per_symbol, MSB_FIRST)
    -> map_bb(pre_diff_code) if gray_coded -> diff_encoder_bb(2^bits_per_symbol) if differential ->
    chunks_to_symbols_bc(points) -> pfb_arb_resampler_ccf(samples_per_symbol, root raised cosine, 32).  work(bytes)
    takes NEW bytes only, streams x n_bytes back to back, and returns the samples they complete, streams x produced;
    the output depends on the concatenated input alone.  engine() 1 (the default) is the fused kernel, 0 runs the
    blocks in a row; MODE_GENERIC is the reference bit for bit in both."""
    _name = "generic_mod"
    _in, _out = np.uint8, np.complex64

    def __init__(self, constellation, samples_per_symbol=2, differential=True, excess_bw=0.35, gray_coded=True, device=0):
        _Block.__init__(self)
        self._create(constellation.base()._h, float(samples_per_symbol), int(bool(differential)), float(excess_bw),
                     int(bool(gray_coded)), int(device))

    def engine(self):
        return self._call("engine")

    def set_engine(self, engine):
        self._call("set_engine", int(engine))

    def bits_per_symbol(self):
        return self._call("bits_per_symbol")

    def samples_per_symbol(self):
        return self._fn("samples_per_symbol")(self._h)          # the float itself, not a status

    def ntaps(self):
        return self._call("ntaps")

    def taps(self):
        t = np.zeros(self.ntaps(), np.float32)
        self._call("taps", _ptr(t), len(t))
        return t

    def max_produced(self, n_bytes):
        """the items per stream that the next work call of n_bytes produces"""
        return self._call("max_produced", int(n_bytes))

    def work(self, input_items, n_bytes=None):
        x, n_bytes = self._work_in(input_items, n_bytes)
        cap = self.max_produced(n_bytes)
        (p_out,), (out,) = self._work_out(cap)
        produced = C.c_longlong(0)
        self._call("work", n_bytes, _ptr(x), p_out, cap, C.byref(produced))
        return out[:produced.value * self._streams]

    def work_device(self, n_bytes, d_in, d_out, out_stride_items, out_capacity, stream=None):
        """device buffers, queued on `stream`; returns the items produced per stream, known at once"""
        produced = C.c_longlong(0)
        self._call("work_device", int(n_bytes), _devptr(d_in), _devptr(d_out), int(out_stride_items), int(out_capacity),
                   C.byref(produced), _stream(stream))
        return produced.value


class psk_mod(generic_mod):
    """digital.psk_mod (psk.py:76-93)"""

    def __init__(self, constellation_points=4, mod_code="gray", **kw):
        generic_mod.__init__(self, psk_constellation(constellation_points, mod_code), **kw)


class qam_mod(generic_mod):
    """digital.qam_mod (qam.py:176-196): the Gray coding is in the constellation; differential is forwarded"""

    def __init__(self, constellation_points=16, differential=True, mod_code="none", **kw):
        generic_mod.__init__(self, qam_constellation(constellation_points, differential, mod_code), differential=differential, **kw)


class bpsk_mod(generic_mod):
    """digital.bpsk_mod (bpsk.py:52-71)"""

    def __init__(self, constellation_points=2, differential=False, **kw):
        if constellation_points != 2:
            raise ValueError("Number of constellation points must be 2 for BPSK.")
        generic_mod.__init__(self, constellation_bpsk(), differential=differential, **kw)


class dbpsk_mod(generic_mod):
    """digital.dbpsk_mod (bpsk.py:114-135): differential is forced"""

    def __init__(self, constellation_points=2, differential=True, **kw):
        if constellation_points != 2:
            raise ValueError("Number of constellation points must be 2 for DBPSK.")
        generic_mod.__init__(self, constellation_bpsk(), differential=True, **kw)


class qpsk_mod(generic_mod):
    """digital.qpsk_mod (qpsk.py:51-75)"""

    def __init__(self, constellation_points=4, gray_coded=True, **kw):
        if constellation_points != 4:
            raise ValueError("QPSK can only have 4 constellation points.")
        if not gray_coded:
            raise ValueError("This QPSK mod/demod works only for gray-coded constellations.")
        generic_mod.__init__(self, constellation_qpsk(), gray_coded=gray_coded, **kw)


class dqpsk_mod(generic_mod):
    """digital.dqpsk_mod (qpsk.py:118-141): differential is forced"""

    def __init__(self, constellation_points=4, gray_coded=True, differential=True, **kw):
        if constellation_points != 4:
            raise ValueError("Number of constellation points must be 4 for DQPSK.")
        generic_mod.__init__(self, constellation_dqpsk(), gray_coded=gray_coded, differential=True, **kw)


# ----------------------------------------------------------------------------
# the scramblers (general/gr_scrambler_bb.i, gr_descrambler_bb.i, gr_additive_scrambler_bb.i) and the packet layer
# (gr-digital/python/packet_utils.py, crc.py, gr-digital/swig/digital_crc32.i)
# ----------------------------------------------------------------------------
class scrambler_bb(_byte_block):
    """gr.scrambler_bb(mask, seed, len): out = the register's bit 0; parity(reg & mask) ^ (in & 1) enters at bit len.
    The register is kept per stream across calls.  MODE_GENERIC walks serially, every other mode is a scan; the bytes
    are the same."""
    _name = "scrambler_bb"

    def __init__(self, mask, seed, len, device=0):
        _Block.__init__(self)
        self._create(C.c_int(int(mask) & 0xffffffff).value, C.c_int(int(seed) & 0xffffffff).value, int(len), int(device))


class descrambler_bb(scrambler_bb):
    """gr.descrambler_bb(mask, seed, len): out = parity(reg & mask) ^ (in & 1); in & 1 enters at bit len"""
    _name = "descrambler_bb"


class additive_scrambler_bb(_byte_block):
    """gr.additive_scrambler_bb(mask, seed, len, count=0): out = in ^ the register's bit 0 (the whole byte is XORed
    with the bit); the register is the seed again after every `count` items if count > 0"""
    _name = "additive_scrambler_bb"

    def __init__(self, mask, seed, len, count=0, device=0):
        _Block.__init__(self)
        self._create(C.c_int(int(mask) & 0xffffffff).value, C.c_int(int(seed) & 0xffffffff).value, int(len), int(count),
                     int(device))


# ----------------------------------------------------------------------------
# the continuous-phase transmitter (general/gr_frequency_modulator_fc.i, gr_bytes_to_syms.i, gr_char_to_float.i,
# gengen/gr_chunks_to_symbols_bf.i, general/gr_cpm.i, gr-digital/swig/digital_cpmmod_bc.i, digital_gmskmod_bc.i,
# gr-digital/python/gmsk.py)
# ----------------------------------------------------------------------------
CPM_LRC, CPM_LSRC, CPM_LREC, CPM_TFM, CPM_GAUSSIAN = range(5)       # gr.cpm.LRC ... gr.cpm.GAUSSIAN


def _designed(fn, *args):
    """the taps of a designer entry: ask for the count, then for the floats"""
    n = _check(fn(*(args + (C.c_void_p(0), 0))))
    t = np.zeros(n, np.float32)
    _check(fn(*(args + (_ptr(t), n))))
    return t


def cpm_phase_response(type, samples_per_sym, L, beta=0.3):
    """gr.cpm.phase_response(type, samples_per_sym, L, beta=0.3): host arithmetic, no device"""
    return _designed(lib().grhip_cpm_phase_response, int(type), int(samples_per_sym), int(L), float(beta))


def firdes_gaussian(gain, spb, bt, ntaps):
    """gr.firdes.gaussian(gain, spb, bt, ntaps): host arithmetic, no device"""
    return _designed(lib().grhip_firdes_gaussian, float(gain), float(spb), float(bt), int(ntaps))


def gmsk_mod_taps(samples_per_symbol, bt):
    """the taps of gmsk_mod's interpolator (gmsk.py:99-107): gaussian(1, sps, bt, 4 sps) convolved with sps ones"""
    return _designed(lib().grhip_gmsk_mod_taps, int(samples_per_symbol), float(bt))


class frequency_modulator_fc(_stream_block):
    """gr.frequency_modulator_fc(sensitivity): phase += sensitivity * in in double, out = (cos, sin) of (float)phase;
    after the last item of a work call |phase| > 16 pi is brought back by whole turns, so the output depends on where
    the calls are cut, as the reference's does.  MODE_GENERIC walks serially and keeps the reference's phase bit for
    bit; every other mode is a scan within 1e-5 + 2^-50 sum|sensitivity * in| of the double evaluation."""
    _name = "frequency_modulator_fc"
    _in, _out = np.float32, np.complex64

    def __init__(self, sensitivity, device=0):
        _Block.__init__(self)
        self._create(float(sensitivity), int(device))

    def set_sensitivity(self, sens):
        self._call("set_sensitivity", float(sens))

    def sensitivity(self):
        return self._fn("sensitivity")(self._h)                     # the float itself, not a status

    def phase(self, stream=0):
        return self._stream_value("phase", C.c_double, stream)

    def set_phase(self, phase):
        self._call("set_phase", float(phase))


class _byte_to_float(_stream_block):
    """streams x n bytes back to back in, per_byte() floats out for each"""
    _view, _out = True, np.float32

    def __init__(self, device=0):
        _Block.__init__(self)
        self._create(int(device))

    def per_byte(self):
        return self._per_out


class bytes_to_syms(_byte_to_float):
    """gr.bytes_to_syms(): eight floats -1 / +1 per byte, bit 7 first"""
    _name = "bytes_to_syms"
    _per_out = 8

    def interpolation(self):
        return 8


class char_to_float(_byte_to_float):
    """gr.char_to_float(): (float)(signed char)"""
    _name = "char_to_float"


class chunks_to_symbols_bf(_byte_to_float):
    """gr.chunks_to_symbols_bf(symbol_table, D=1): n bytes in, n * D floats out per stream,
    symbol_table[in * D : in * D + D]; an index outside the table gives zeros"""
    _name = "chunks_to_symbols_bf"

    def __init__(self, symbol_table, D=1, device=0):
        _Block.__init__(self)
        t = np.ascontiguousarray(symbol_table, dtype=np.float32).reshape(-1)    # owns the memory until the call returns
        self._create(_ptr(t) if len(t) else C.c_void_p(0), len(t), int(D), int(device))

    def D(self):
        return self._call("D")

    per_byte, _per_out = D, property(D)


class _cpm_hier(_Block):
    """one handle for char_to_float / bytes_to_syms -> interp_fir_filter_fff -> frequency_modulator_fc on NEW items
    only: streams x n items back to back in, streams x n * items_out() complex items out.  A work call is a work call
    of every inner block (the modulator's wrap falls at its end).  engine() 1 is the fused kernel (the default outside
    MODE_GENERIC where the taps fit), 0 the blocks in a row."""
    _view, _out = True, np.complex64
    _per_item = 1           # symbols per input item

    def engine(self):
        return self._call("engine")

    def set_engine(self, engine):
        self._call("set_engine", int(engine))

    def samples_per_symbol(self):
        return self._call("samples_per_symbol")

    def items_out(self):
        return self._per_item * self.samples_per_symbol()

    _per_out = property(items_out)

    def taps(self):
        return _designed(self._fn("filter_taps"), self._h)

    def phase(self, stream=0):
        return self._stream_value("phase", C.c_double, stream)

    def work(self, input_items, n=None, want_freq=False):
        return self._stream_work(input_items, n, [np.float32], want_freq)

    def work_device(self, n, d_in, d_out, d_freq=None, stream=None):
        """device buffers, queued on `stream`; d_freq (optional) takes the frequency samples"""
        return self._call("work_device", int(n), _devptr(d_in), _devptr(d_out), _devptr(d_freq), _stream(stream))


class cpmmod_bc(_cpm_hier):
    """digital.cpmmod_bc(type, h, samples_per_sym, L, beta=0.3): signed-char symbols in"""
    _name = "cpmmod_bc"

    def __init__(self, type, h, samples_per_sym, L, beta=0.3, device=0):
        _Block.__init__(self)
        self._create(int(type), float(h), int(samples_per_sym), int(L), float(beta), int(device))

    @staticmethod
    def tile():
        return lib().grhip_cpmmod_bc_tile()


class gmskmod_bc(_cpm_hier):
    """digital.gmskmod_bc(samples_per_sym=2, bt=0.3, L=4): cpmmod_bc(GAUSSIAN, 0.5, samples_per_sym, L, bt)"""
    _name = "gmskmod_bc"

    def __init__(self, samples_per_sym=2, bt=0.3, L=4, device=0):
        _Block.__init__(self)
        self._create(int(samples_per_sym), float(bt), int(L), int(device))


class gmsk_mod(_cpm_hier):
    """digital.gmsk_mod(samples_per_symbol=2, bt=0.35) of gmsk.py: bytes in, eight symbols each"""
    _name = "gmsk_mod"
    _per_item = 8

    def __init__(self, samples_per_symbol=2, bt=0.35, device=0):
        _Block.__init__(self)
        if int(samples_per_symbol) != samples_per_symbol:           # gmsk.py:84 truncates; a fraction is refused here
            raise ValueError("samples_per_symbol must be an integer >= 2, is %r" % (samples_per_symbol,))
        self._create(int(samples_per_symbol), float(bt), int(device))

    @staticmethod
    def bits_per_symbol():
        return 1


def frequency_modulator_fc_tile():
    """items per workgroup of frequency_modulator_fc's scan: calls at or below it are one launch"""
    return lib().grhip_frequency_modulator_fc_tile()


# ----------------------------------------------------------------------------
# gr-trellis (gr-trellis/src/lib/fsm.i, trellis.i): fsm, trellis_encoder_XX, trellis_metrics_X,
# trellis_constellation_metrics_cf, trellis_viterbi_X
# ----------------------------------------------------------------------------
TRELLIS_EUCLIDEAN, TRELLIS_HARD_SYMBOL, TRELLIS_HARD_BIT = 200, 201, 202       # digital_metric_type.h:26-28


def _ints(v):
    return np.ascontiguousarray(v, dtype=np.int32).reshape(-1)


class fsm(object):
    """trellis.fsm: a host object, no device needed.  The reference's constructors by their arguments:
    fsm(I, S, O, NS, OS); fsm(name) with the path of an .fsm file (fsm(text=...) takes the file's text);
    fsm(k, n, G) the binary convolutional code; fsm(mod_size, ch_length) ISI; fsm(P, M, L) CPM;
    fsm(FSM1, FSM2) the joint trellis; fsm(FSM, n) radix-n; fsm(FSM) a copy."""

    def __init__(self, *args, **kw):
        self._h = C.c_void_p(0)
        L = lib()
        h = C.byref(self._h)
        if kw:
            if args or list(kw) != ["text"]:
                raise TypeError("fsm(text=...) takes nothing else")
            _check(L.grhip_fsm_create_text(h, str(kw["text"]).encode()))
        elif len(args) == 5:
            ns, os_ = _ints(args[3]), _ints(args[4])
            _check(L.grhip_fsm_create(h, int(args[0]), int(args[1]), int(args[2]), _ptr(ns), len(ns), _ptr(os_), len(os_)))
        elif len(args) == 1 and isinstance(args[0], fsm):
            f = args[0]
            ns, os_ = f.NS(), f.OS()
            _check(L.grhip_fsm_create(h, f.I(), f.S(), f.O(), _ptr(ns), len(ns), _ptr(os_), len(os_)))
        elif len(args) == 1:
            _check(L.grhip_fsm_create_file(h, os.fsencode(args[0])))
        elif len(args) == 2 and isinstance(args[0], fsm) and isinstance(args[1], fsm):
            _check(L.grhip_fsm_create_joint(h, args[0]._h, args[1]._h))
        elif len(args) == 2 and isinstance(args[0], fsm):
            _check(L.grhip_fsm_create_radix(h, args[0]._h, int(args[1])))
        elif len(args) == 2:
            _check(L.grhip_fsm_create_isi(h, int(args[0]), int(args[1])))
        elif len(args) == 3 and np.ndim(args[2]) > 0:
            g = _ints(args[2])
            _check(L.grhip_fsm_create_generator(h, int(args[0]), int(args[1]), _ptr(g), len(g)))
        elif len(args) == 3:
            _check(L.grhip_fsm_create_cpm(h, int(args[0]), int(args[1]), int(args[2])))
        else:
            raise TypeError("fsm: no constructor takes %d arguments" % len(args))

    def __del__(self):
        try:
            if self._h:
                lib().grhip_fsm_destroy(self._h)
                self._h = C.c_void_p(0)
        except Exception:
            pass

    def _int(self, name):
        return _check(getattr(lib(), "grhip_fsm_" + name)(self._h))

    def _table(self, name, *state):
        fn = getattr(lib(), "grhip_fsm_" + name)
        n = _check(fn(self._h, *(state + (C.c_void_p(0), 0))))
        a = np.zeros(max(n, 1), np.int32)
        _check(fn(self._h, *(state + (_ptr(a), n))))
        return a[:n]

    def I(self):
        return self._int("I")

    def S(self):
        return self._int("S")

    def O(self):
        return self._int("O")

    def connected(self):
        """False where the reference prints "FSM appears to be disconnected" """
        return bool(self._int("connected"))

    def NS(self):
        return self._table("NS")

    def OS(self):
        return self._table("OS")

    def PS(self):
        return [self._table("PS", j) for j in range(self.S())]

    def PI(self):
        return [self._table("PI", j) for j in range(self.S())]

    def TMl(self):
        return self._table("TMl")

    def TMi(self):
        return self._table("TMi")


class trellis_encoder_bb(_byte_block):
    """trellis.encoder_bb(FSM, ST): out[i] = OS[ST * I + in[i]], ST = NS[ST * I + in[i]]; one state per stream, kept
    across calls.  An input outside [0, I) is refused and leaves the states alone."""
    _name = "trellis_encoder_bb"

    def __init__(self, FSM, ST, device=0):
        _Block.__init__(self)
        self._create(FSM._h, int(ST), int(device))

    def ST(self, stream=0):
        return self._stream_value("ST", C.c_int, stream)

    def set_ST(self, ST):
        self._call("set_ST", int(ST))


class trellis_encoder_bs(trellis_encoder_bb):
    _name = "trellis_encoder_bs"
    _out = np.int16


class trellis_encoder_bi(trellis_encoder_bb):
    _name = "trellis_encoder_bi"
    _out = np.int32


class trellis_encoder_ss(trellis_encoder_bb):
    _name = "trellis_encoder_ss"
    _in = np.int16
    _out = np.int16


class trellis_encoder_si(trellis_encoder_bb):
    _name = "trellis_encoder_si"
    _in = np.int16
    _out = np.int32


class trellis_encoder_ii(trellis_encoder_bb):
    _name = "trellis_encoder_ii"
    _in = np.int32
    _out = np.int32


class trellis_metrics_f(_stream_block):
    """trellis.metrics_f(O, D, TABLE, TYPE): n steps of D items in, O floats per step out, the reference bit for bit.
    TYPE is TRELLIS_EUCLIDEAN or TRELLIS_HARD_SYMBOL; anything else is refused here, where the reference throws in work."""
    _name = "trellis_metrics_f"
    _in = np.float32
    _out = np.float32

    def __init__(self, O, D, TABLE, TYPE, device=0):
        _Block.__init__(self)
        t = np.ascontiguousarray(TABLE, dtype=self._in).reshape(-1)
        self._create(int(O), int(D), _ptr(t), len(t), int(TYPE), int(device))
        self._per_in, self._per_out = int(D), int(O)

    def set_TABLE(self, TABLE):
        t = np.ascontiguousarray(TABLE, dtype=self._in).reshape(-1)
        self._call("set_TABLE", _ptr(t), len(t))

    def O(self):
        return self._call("O")

    def D(self):
        return self._call("D")

    def TYPE(self):
        return self._call("TYPE")


class trellis_metrics_s(trellis_metrics_f):
    _name = "trellis_metrics_s"
    _in = np.int16


class trellis_metrics_i(trellis_metrics_f):
    _name = "trellis_metrics_i"
    _in = np.int32


class trellis_metrics_c(trellis_metrics_f):
    _name = "trellis_metrics_c"
    _in = np.complex64


class trellis_constellation_metrics_cf(_stream_block):
    """trellis.constellation_metrics_cf(constellation, TYPE): the constellation's calc_metric, dimensionality() complex
    items per step in, arity() floats out"""
    _name = "trellis_constellation_metrics_cf"
    _in = np.complex64
    _out = np.float32

    def __init__(self, constellation, TYPE, device=0):
        _Block.__init__(self)
        self._create(constellation.base()._h, int(TYPE), int(device))
        self._per_in, self._per_out = self.D(), self.O()

    def O(self):
        return self._call("O")

    def D(self):
        return self._call("D")

    def TYPE(self):
        return self._call("TYPE")


class trellis_viterbi_b(_byte_block):
    """trellis.viterbi_b(FSM, K, S0, SK): n * O floats in, n symbols out per stream, n a multiple of K; every block of
    K steps is viterbi_algorithm's output byte for byte in every mode"""
    _name = "trellis_viterbi_b"
    _in = np.float32

    def __init__(self, FSM, K, S0, SK, device=0):
        _Block.__init__(self)
        self._create(FSM._h, int(K), int(S0), int(SK), int(device))
        self._per_in = FSM.O()

    def K(self):
        return self._call("K")

    def _state(self, name):
        v = C.c_int(0)
        self._call(name, C.byref(v))
        return v.value

    def S0(self):
        return self._state("S0")

    def SK(self):
        return self._state("SK")

    def trace_window(self):
        """the steps whose trace fits in LDS; a larger K goes through the workspace"""
        return self._call("trace_window")

    def resident_blocks(self):
        """the blocks decoded at once; a call with more has its persistent wavefronts take further ones"""
        return self._call("resident_blocks")

    def blocks_per_wavefront(self):
        return self._call("blocks_per_wavefront")

    def workspace_bytes(self):
        v = C.c_ulonglong(0)
        self._call("workspace_bytes", C.byref(v))
        return v.value

    def dead_ends(self):
        """steps at which the traceback stood in a state without predecessors, over the handle's life"""
        v = C.c_longlong(0)
        self._call("dead_ends", C.byref(v))
        return v.value


class trellis_viterbi_s(trellis_viterbi_b):
    _name = "trellis_viterbi_s"
    _out = np.int16


class trellis_viterbi_i(trellis_viterbi_b):
    _name = "trellis_viterbi_i"
    _out = np.int32


class _trellis_viterbi_combined(trellis_viterbi_b):
    """trellis.viterbi_combined_XX(FSM, K, S0, SK, D, TABLE, TYPE): the metrics of trellis_metrics_X computed per step
    inside the decoder; n * D items in, n symbols out per stream.  engine() 1 (the default) forms the metrics in the
    decoder's LDS window, 0 runs the metrics kernel and then the decoder; MODE_GENERIC runs engine 0.  The symbols are
    the reference's in both."""

    def __init__(self, FSM, K, S0, SK, D, TABLE, TYPE, device=0):
        _Block.__init__(self)
        t = np.ascontiguousarray(TABLE, dtype=self._in).reshape(-1)
        self._create(FSM._h, int(K), int(S0), int(SK), int(D), _ptr(t), len(t), int(TYPE), int(device))
        self._per_in = int(D)

    def set_TABLE(self, TABLE):
        t = np.ascontiguousarray(TABLE, dtype=self._in).reshape(-1)
        self._call("set_TABLE", _ptr(t), len(t))

    def set_engine(self, engine):
        self._call("set_engine", int(engine))

    def engine(self):
        return self._call("engine")

    def D(self):
        return self._call("D")

    def TYPE(self):
        return self._call("TYPE")


class trellis_viterbi_combined_sb(_trellis_viterbi_combined):
    _name = "trellis_viterbi_combined_sb"
    _in = np.int16


class trellis_viterbi_combined_ss(_trellis_viterbi_combined):
    _name = "trellis_viterbi_combined_ss"
    _in = np.int16
    _out = np.int16


class trellis_viterbi_combined_si(_trellis_viterbi_combined):
    _name = "trellis_viterbi_combined_si"
    _in = np.int16
    _out = np.int32


class trellis_viterbi_combined_ib(_trellis_viterbi_combined):
    _name = "trellis_viterbi_combined_ib"
    _in = np.int32


class trellis_viterbi_combined_is(_trellis_viterbi_combined):
    _name = "trellis_viterbi_combined_is"
    _in = np.int32
    _out = np.int16


class trellis_viterbi_combined_ii(_trellis_viterbi_combined):
    _name = "trellis_viterbi_combined_ii"
    _in = np.int32
    _out = np.int32


class trellis_viterbi_combined_fb(_trellis_viterbi_combined):
    _name = "trellis_viterbi_combined_fb"


class trellis_viterbi_combined_fs(_trellis_viterbi_combined):
    _name = "trellis_viterbi_combined_fs"
    _out = np.int16


class trellis_viterbi_combined_fi(_trellis_viterbi_combined):
    _name = "trellis_viterbi_combined_fi"
    _out = np.int32


class trellis_viterbi_combined_cb(_trellis_viterbi_combined):
    _name = "trellis_viterbi_combined_cb"
    _in = np.complex64


class trellis_viterbi_combined_cs(_trellis_viterbi_combined):
    _name = "trellis_viterbi_combined_cs"
    _in = np.complex64
    _out = np.int16


class trellis_viterbi_combined_ci(_trellis_viterbi_combined):
    _name = "trellis_viterbi_combined_ci"
    _in = np.complex64
    _out = np.int32


def random_mask_vec8():
    """packet_utils.random_mask_vec8: the 4096 whitening bytes, generated by the library"""
    t = np.zeros(4096, np.uint8)
    _check(lib().grhip_whitening_table(_ptr(t), 4096))
    return t


default_access_code = "".join("{:08b}".format(b) for b in (0xAC, 0xDD, 0xA4, 0xE2, 0xF2, 0x8C, 0x20, 0xFC))   # packet_utils.py:72-73


class crc32(_Block):
    """digital.crc32 / digital.update_crc32 on the device: polynomial 0x04C11DB7, MSB first, start and final XOR
    0xFFFFFFFF.  crc32(bytes) and update_crc32(crc, bytes) stage a host buffer; the _device forms take an address
    or a tensor and a length."""
    _name = "crc32"

    def __init__(self, device=0):
        _Block.__init__(self)
        self._create(int(device))

    def set_segment_bytes(self, nbytes):
        """tuning: bytes one workgroup takes in a row (0 = chosen per call); results do not depend on it"""
        self._call("set_segment_bytes", int(nbytes))

    @staticmethod
    def _bytes(s):
        return np.frombuffer(s, np.uint8) if isinstance(s, (bytes, bytearray)) else np.ascontiguousarray(s, dtype=np.uint8).reshape(-1)

    def crc32(self, s):
        x, out = self._bytes(s), C.c_uint(0)
        self._call("compute", _ptr(x) if len(x) else C.c_void_p(0), len(x), C.byref(out))
        return out.value

    def update_crc32(self, crc, s):
        x, out = self._bytes(s), C.c_uint(0)
        self._call("update", int(crc) & 0xffffffff, _ptr(x) if len(x) else C.c_void_p(0), len(x), C.byref(out))
        return out.value

    def crc32_device(self, d_buf, n, stream=None):
        out = C.c_uint(0)
        self._call("compute_device", _devptr(d_buf), int(n), C.byref(out), _stream(stream))
        return out.value

    def update_crc32_device(self, crc, d_buf, n, stream=None):
        out = C.c_uint(0)
        self._call("update_device", int(crc) & 0xffffffff, _devptr(d_buf), int(n), C.byref(out), _stream(stream))
        return out.value


PACKET_JOB = np.dtype([("whitener_offset", np.uint32), ("length", np.uint32), ("in_offset", np.uint32), ("out_offset", np.uint32)])
PACKET_REC = np.dtype([("whitener_offset", np.uint32), ("length", np.uint32), ("offset", np.uint32), ("reserved", np.uint32)])


class packet_maker(_Block):
    """packet_utils.make_packet for many payloads in one call: preamble, access code, doubled header, payload + CRC-32
    (whitened from whitener_offset), 0x55 and the padding of pad_for_usrp.  make_packets(payloads, whitener_offsets)
    returns the packets as bytes; plan() and work_device() are the same on device buffers."""
    _name = "packet_maker"

    def __init__(self, samples_per_symbol, bits_per_symbol, access_code=default_access_code, pad_for_usrp=True, whitening=True,
                 device=0):
        _Block.__init__(self)
        if not isinstance(access_code, str):
            raise ValueError("access_code must be a string containing only 0's and 1's (%r)" % (access_code,))
        self._create(C.c_char_p(access_code.encode()), float(samples_per_symbol), int(bits_per_symbol), int(bool(pad_for_usrp)),
                     int(bool(whitening)), int(device))

    def packet_bytes(self, payload_len):
        return self._call("packet_bytes", int(payload_len))

    def plan(self, lengths, whitener_offsets=None):
        """(jobs as a PACKET_JOB array, payload bytes in all, packet bytes in all)"""
        ln = np.ascontiguousarray(lengths, dtype=np.int32).reshape(-1)
        wo = None if whitener_offsets is None else np.ascontiguousarray(whitener_offsets, dtype=np.int32).reshape(-1)
        if wo is not None and len(wo) != len(ln):
            raise ValueError("one whitener offset per payload")
        jobs = np.zeros(max(len(ln), 1), PACKET_JOB)
        tin, tout = C.c_longlong(0), C.c_longlong(0)
        self._call("plan", len(ln), _ptr(ln), C.c_void_p(0) if wo is None else _ptr(wo), _ptr(jobs), C.byref(tin), C.byref(tout))
        return jobs[:len(ln)], tin.value, tout.value

    def work_device(self, n, d_jobs, d_payloads, d_out, stream=None):
        return self._call("work_device", int(n), _devptr(d_jobs), _devptr(d_payloads), _devptr(d_out), _stream(stream))

    def make_packets(self, payloads, whitener_offsets=None):
        """payloads: a list of bytes; returns the list of packets"""
        jobs, tin, tout = self.plan([len(p) for p in payloads], whitener_offsets)
        ln = np.ascontiguousarray(jobs["length"], dtype=np.int32)
        wo = np.ascontiguousarray(jobs["whitener_offset"], dtype=np.int32)
        x = np.frombuffer(b"".join(bytes(p) for p in payloads) + b"\0", np.uint8)
        out = np.zeros(max(tout, 1), np.uint8)
        total = C.c_longlong(0)
        self._call("work", len(ln), _ptr(ln), _ptr(wo), _ptr(x), _ptr(out), int(tout), C.byref(total))
        ends = list(jobs["out_offset"][1:]) + [total.value]
        return [out[int(a):int(b)].tobytes() for a, b in zip(jobs["out_offset"], ends)]


class packet_check(_Block):
    """packet_utils.unmake_packet for messages on the device: dewhiten, compare the CRC-32, one ok byte per message"""
    _name = "packet_check"

    def __init__(self, device=0):
        _Block.__init__(self)
        self._create(int(device))

    def work_device(self, n_streams, max_msgs, d_recs, rec_stride, d_counts, count_stride_words, d_pool, pool_stride, dewhitening,
                    d_payload_out, d_ok, stream=None):
        return self._call("work_device", int(n_streams), int(max_msgs), _devptr(d_recs), int(rec_stride), _devptr(d_counts),
                          int(count_stride_words), _devptr(d_pool), int(pool_stride), int(bool(dewhitening)), _devptr(d_payload_out),
                          _devptr(d_ok), _stream(stream))


# ----------------------------------------------------------------------------
# gr.iir_filter_ffd, blks2.fm_deemph, gr.firdes.low_pass  (filter/gr_iir_filter_ffd.i, blks2impl/fm_emph.py,
# general/gr_firdes.i)
# ----------------------------------------------------------------------------
def _taps_d(taps):
    t = np.ascontiguousarray(taps, dtype=np.float64).reshape(-1)
    return t, (_ptr(t) if len(t) else C.c_void_p(0)), len(t)


class iir_filter_ffd(_stream_block):
    """gr.iir_filter_ffd(fftaps, fbtaps): y[t] = sum ff[i] x[t-i] + sum_{i>=1} fb[i] y[t-i] in double (the feedback is
    added, fbtaps[0] is never read), float in and out.  work(x) takes streams x n_in items back to back and returns
    as many; the delay lines carry across calls.  MODE_GENERIC is the reference's recurrence bit for bit; every other
    mode runs calls of more than chunk() items in chunks where the taps allow it (chunked()).  set_taps is latched:
    it holds, with zeroed delay lines, from the next work call.  work_device does not synchronise."""
    _name = "iir_filter_ffd"
    _in = _out = np.float32

    def __init__(self, fftaps, fbtaps, device=0):
        _Block.__init__(self)
        f, pf, n = _taps_d(fftaps)          # f and b own the memory until the call returns
        b, pb, m = _taps_d(fbtaps)
        self._create(pf, n, pb, m, int(device))

    def set_taps(self, fftaps, fbtaps):
        f, pf, n = _taps_d(fftaps)
        b, pb, m = _taps_d(fbtaps)
        self._call("set_taps", pf, n, pb, m)

    def chunked(self):
        """True if the next call of more than chunk() items takes the chunked form"""
        return bool(self._call("chunked"))

    def work(self, input_items, n_in=None):
        return self._stream_work(input_items, n_in)

    @staticmethod
    def chunk():
        """items per chunk of the chunked form"""
        return lib().grhip_iir_filter_ffd_chunk()


def fm_deemph_taps(fs, tau=75e-6):
    """(btaps, ataps) of blks2.fm_deemph(fs, tau), two float64 each: host arithmetic only, no device needed"""
    b = np.zeros(2, np.float64)
    a = np.zeros(2, np.float64)
    _check(lib().grhip_fm_deemph_taps(float(fs), float(tau), _ptr(b), _ptr(a)))
    return b, a


class fm_deemph(iir_filter_ffd):
    """blks2.fm_deemph(fs, tau=75e-6) (blks2impl/fm_emph.py:44-72): gr.iir_filter_ffd over fm_deemph_taps(fs, tau)"""

    def __init__(self, fs, tau=75e-6, device=0):
        b, a = fm_deemph_taps(fs, tau)
        iir_filter_ffd.__init__(self, b, a, device)


def firdes_low_pass(gain, sampling_freq, cutoff_freq, transition_width, window=0, beta=6.76):
    """gr.firdes.low_pass(gain, sampling_freq, cutoff_freq, transition_width, window=WIN_HAMMING, beta=6.76): host
    arithmetic only, no device needed.  A failed argument check is a GrhipError."""
    args = (float(gain), float(sampling_freq), float(cutoff_freq), float(transition_width), int(window), float(beta))
    n = C.c_size_t(0)
    rc = lib().grhip_firdes_low_pass(*(args + (C.c_void_p(0), 0, C.byref(n))))
    if rc != -2:                                    # GRHIP_ERANGE: the size query's answer
        _check(rc)
    out = np.zeros(max(n.value, 1), dtype=np.float32)
    _check(lib().grhip_firdes_low_pass(*(args + (_ptr(out), n.value, C.byref(n)))))
    return out[:n.value]


class _demod_cf(_Block):
    """what the fused FM and AM receivers share: streams x n_in NEW complex items in, streams x produced floats out"""
    _in, _out = np.complex64, np.float32

    def produced(self, n_in):
        """outputs per stream of the next work call of n_in items"""
        return self._call("produced", int(n_in))

    def engine(self):
        """1: the fused kernel runs the next call; 0: the three blocks in a row"""
        return self._call("engine")

    def work(self, input_items, n_in=None):
        x, n_in = self._work_in(input_items, n_in)
        got = C.c_int(0)
        (p_out,), (out,) = self._work_out(self.produced(n_in))
        self._call("work", n_in, _ptr(x) if len(x) else C.c_void_p(0), p_out, C.byref(got))
        return out[:got.value * self._streams]

    def work_device(self, n_in, d_in, d_out, d_produced=None, stream=None):
        """work on device buffers, queued on `stream`; d_produced: a device int that receives the count, or None"""
        return self._call("work_device", int(n_in), _devptr(d_in), _devptr(d_out), _devptr(d_produced), _stream(stream))


class fm_demod_cf(_demod_cf):
    """blks2.fm_demod_cf (blks2impl/fm_demod.py:51-72) as one handle: quadrature_demod_cf(channel_rate / (2 pi deviation))
    -> fm_deemph(channel_rate, tau) (tau=None: none) -> fir_filter_fff(audio_decim, audio_taps).  The reference designs
    its audio taps with optfir.low_pass; this constructor takes them as given, and design(...) designs them as the
    reference does (optfir_low_pass).  work(x) takes
    streams x n_in NEW complex items back to back (no history in front) and returns streams x produced floats, stream
    s from s * produced; every inner block starts from a zero history and carries its state across calls.
    MODE_GENERIC is the reference's chain bit for bit; every other mode runs one fused kernel where engine() is 1."""
    _name = "fm_demod_cf"

    def __init__(self, channel_rate, audio_decim, deviation, audio_taps, tau=75e-6, device=0):
        _Block.__init__(self)
        k = channel_rate / (2 * math.pi * deviation)
        b, a = fm_deemph_taps(channel_rate, tau) if tau is not None else ((), ())
        f, pf, n = _taps_d(b)
        fb, pb, m = _taps_d(a)
        t = np.ascontiguousarray(audio_taps, dtype=np.float32).reshape(-1)
        if int(audio_decim) != audio_decim:
            raise ValueError("audio_decim must be an integer")
        self._create(float(k), pf, n, pb, m, int(audio_decim), _ptr(t), len(t), int(device))
        self.audio_taps, self.audio_decim, self.k = t, int(audio_decim), float(np.float32(k))

    @classmethod
    def design(cls, channel_rate, audio_decim, deviation, audio_pass, audio_stop, gain=1.0, tau=75e-6, device=0):
        """blks2.fm_demod_cf(channel_rate, audio_decim, deviation, audio_pass, audio_stop, gain, tau) with the
        reference's own audio filter: optfir.low_pass(gain, channel_rate, audio_pass, audio_stop, 0.1, 60), narrowed
        to float per tap (blks2impl/fm_demod.py:60-66)"""
        taps = optfir_low_pass(gain, channel_rate, audio_pass, audio_stop, 0.1, 60).astype(np.float32)
        blk = cls.__new__(cls)
        fm_demod_cf.__init__(blk, channel_rate, audio_decim, deviation, taps, tau, device)
        return blk

    @staticmethod
    def tile():
        """input samples per workgroup of the fused kernel"""
        return lib().grhip_fm_demod_cf_tile()


class nbfm_rx(fm_demod_cf):
    """blks2.nbfm_rx(audio_rate, quad_rate, tau=75e-6, max_dev=5e3) (blks2impl/nbfm_rx.py:28-88): the rates as
    integers, quad_rate a multiple of audio_rate (ValueError otherwise), k = quad_rate / (2 pi max_dev), the
    de-emphasis at quad_rate, and the audio taps of firdes.low_pass(1.0, quad_rate, 2.7e3, 0.5e3, WIN_HAMMING)"""

    def __init__(self, audio_rate, quad_rate, tau=75e-6, max_dev=5e3, device=0):
        audio_rate = int(audio_rate)
        quad_rate = int(quad_rate)
        if quad_rate % audio_rate != 0:
            raise ValueError("quad_rate is not an integer multiple of audio_rate")
        taps = firdes_low_pass(1.0, quad_rate, 2.7e3, 0.5e3, WIN_HAMMING)
        fm_demod_cf.__init__(self, quad_rate, quad_rate // audio_rate, max_dev, taps, tau, device)


def demod_20k0f3e_cf(channel_rate, audio_decim, device=0):
    """blks2.demod_20k0f3e_cf (blks2impl/fm_demod.py:74-91): NBFM, 5 kHz deviation, audio 3 kHz / 4.5 kHz"""
    return fm_demod_cf.design(channel_rate, audio_decim, 5000, 3000, 4500, device=device)


def demod_200kf3e_cf(channel_rate, audio_decim, device=0):
    """blks2.demod_200kf3e_cf (blks2impl/fm_demod.py:93-111): WFM, 75 kHz deviation, audio 15 kHz / 16 kHz, gain 20.
    At the receiver's shape (320 kHz, audio_decim 10) the designed filter has 1164 taps, more than the fused FM kernel
    takes: engine() is 0 there and the three blocks run in a row."""
    return fm_demod_cf.design(channel_rate, audio_decim, 75000, 15000, 16000, 20.0, device=device)


# ----------------------------------------------------------------------------
# gr.remez and gnuradio.optfir (general/gr_remez.i, python/gnuradio/optfir.py): host arithmetic only
# ----------------------------------------------------------------------------
_REMEZ_TYPES = {"bandpass": 1, "differentiator": 2, "hilbert": 3}


def _sized_doubles(call):
    """the size query of the tap designers: call(out, cap, ntaps) once for the size, once for the taps"""
    n = C.c_size_t(0)
    rc = call(C.c_void_p(0), 0, C.byref(n))
    if rc != -2 or n.value == 0:                    # GRHIP_ERANGE with a count: the size query's answer
        _check(rc)
    out = np.zeros(max(n.value, 1), dtype=np.float64)
    _check(call(_ptr(out), n.value, C.byref(n)))
    return out[:n.value]


def remez(order, bands, ampl, error_weight=(), filter_type="bandpass", grid_density=16):
    """gr.remez(order, bands, ampl, error_weight, filter_type="bandpass", grid_density=16): order + 1 float64 taps, the
    reference's bit for bit.  A refused argument or a failed exchange is a GrhipError with the reference's message."""
    b, pb, nb = _taps_d(bands)
    a, pa, na = _taps_d(ampl)
    w, pw, nw = _taps_d(error_weight)
    if na != nb:
        raise GrhipError(-1, "gr_remez: must have one response magnitude for each band edge")
    if filter_type not in _REMEZ_TYPES:
        raise GrhipError(-1, "gr_remez: unknown ftype '%s'" % (filter_type,))
    order, kind, density = int(order), _REMEZ_TYPES[filter_type], int(grid_density)
    return _sized_doubles(lambda out, cap, n: lib().grhip_remez(order, pb, nb, pa, pw, nw, kind, density, out, cap, n))


def _optfir(name, args, nextra_taps):
    args = tuple(float(v) for v in args) + (int(nextra_taps),)
    fn = getattr(lib(), "grhip_optfir_" + name)
    return _sized_doubles(lambda out, cap, n: fn(*(args + (out, cap, n))))


def optfir_low_pass(gain, Fs, freq1, freq2, passband_ripple_db, stopband_atten_db, nextra_taps=2):
    """optfir.low_pass: float64 taps as gr.remez returns them"""
    return _optfir("low_pass", (gain, Fs, freq1, freq2, passband_ripple_db, stopband_atten_db), nextra_taps)


def optfir_high_pass(gain, Fs, freq1, freq2, passband_ripple_db, stopband_atten_db, nextra_taps=2):
    """optfir.high_pass: an odd number of taps; the gain is not used, as in the reference"""
    return _optfir("high_pass", (gain, Fs, freq1, freq2, passband_ripple_db, stopband_atten_db), nextra_taps)


def optfir_band_pass(gain, Fs, freq_sb1, freq_pb1, freq_pb2, freq_sb2, passband_ripple_db, stopband_atten_db, nextra_taps=2):
    """optfir.band_pass"""
    return _optfir("band_pass", (gain, Fs, freq_sb1, freq_pb1, freq_pb2, freq_sb2, passband_ripple_db, stopband_atten_db),
                   nextra_taps)


def optfir_band_reject(gain, Fs, freq_pb1, freq_sb1, freq_sb2, freq_pb2, passband_ripple_db, stopband_atten_db, nextra_taps=2):
    """optfir.band_reject: an odd number of taps"""
    return _optfir("band_reject", (gain, Fs, freq_pb1, freq_sb1, freq_sb2, freq_pb2, passband_ripple_db, stopband_atten_db),
                   nextra_taps)


def optfir_spec(kind, gain, Fs, freqs, passband_ripple_db, stopband_atten_db, nextra_taps=2):
    """(order, bands, ampl, weights) that optfir.<kind> hands to gr.remez; kind is "low_pass", "high_pass",
    "band_pass" or "band_reject", freqs its band edges in the reference's order"""
    k = ("low_pass", "high_pass", "band_pass", "band_reject").index(kind)
    f, pf, nf = _taps_d(freqs)
    order, nb = C.c_int(0), C.c_size_t(0)
    bands, ampl, weight = np.zeros(6), np.zeros(6), np.zeros(3)
    _check(lib().grhip_optfir_spec(k, float(gain), float(Fs), pf, nf, float(passband_ripple_db), float(stopband_atten_db),
                                   int(nextra_taps), C.byref(order), _ptr(bands), _ptr(ampl), _ptr(weight), C.byref(nb)))
    return order.value, bands[:2 * nb.value], ampl[:2 * nb.value], weight[:nb.value]


# ----------------------------------------------------------------------------
# blks2.am_demod_cf / demod_10k0a3e_cf (blks2impl/am_demod.py)
# ----------------------------------------------------------------------------
class am_demod_cf(_demod_cf):
    """blks2.am_demod_cf(channel_rate, audio_decim, audio_pass, audio_stop) (blks2impl/am_demod.py:42-58) as one handle:
    complex_to_mag -> add_const_ff(-1) -> fir_filter_fff(audio_decim, audio_taps), the taps those of
    optfir_low_pass(0.5, channel_rate, audio_pass, audio_stop, 0.1, 60) narrowed to float.  work(x) takes streams x n_in
    NEW complex items back to back and returns streams x produced floats, stream s from s * produced; the FIR starts
    from a zero delay line and carries it across calls.  MODE_GENERIC is the reference's chain bit for bit; every
    other mode runs one fused kernel where engine() is 1."""
    _name = "am_demod_cf"

    def __init__(self, channel_rate, audio_decim, audio_pass, audio_stop, device=0):
        taps = optfir_low_pass(0.5, channel_rate, audio_pass, audio_stop, 0.1, 60).astype(np.float32)
        self._init_taps(audio_decim, taps, device)

    @classmethod
    def from_taps(cls, audio_decim, taps, device=0):
        """the same block over given audio taps"""
        blk = cls.__new__(cls)
        am_demod_cf._init_taps(blk, audio_decim, taps, device)
        return blk

    def _init_taps(self, audio_decim, taps, device):
        _Block.__init__(self)
        t = np.ascontiguousarray(taps, dtype=np.float32).reshape(-1)
        if int(audio_decim) != audio_decim:
            raise ValueError("audio_decim must be an integer")
        self._create(int(audio_decim), _ptr(t) if len(t) else C.c_void_p(0), len(t), int(device))
        self.audio_taps, self.audio_decim = t, int(audio_decim)

    @staticmethod
    def tile():
        """input samples per workgroup of the fused kernel"""
        return lib().grhip_am_demod_cf_tile()

    @staticmethod
    def outputs_per_lane():
        """adjacent outputs a lane of the fused kernel forms with audio_decim == 1"""
        return lib().grhip_am_demod_cf_outputs_per_lane()

    @staticmethod
    def max_taps():
        """the longest filter the fused kernel takes"""
        return lib().grhip_am_demod_cf_max_taps()


class demod_10k0a3e_cf(am_demod_cf):
    """blks2.demod_10k0a3e_cf(channel_rate, audio_decim) (blks2impl/am_demod.py:60-76): AM, audio 5 kHz / 5.5 kHz"""

    def __init__(self, channel_rate, audio_decim, device=0):
        am_demod_cf.__init__(self, channel_rate, audio_decim, 5000, 5500, device)


class keep_one_in_n(_Block):
    """gr.keep_one_in_n(item_size, n): work takes the input items as an array whose itemsize is item_size (or as bytes)
    and returns the kept ones; the countdown carries across calls"""
    _name = "keep_one_in_n"

    def __init__(self, item_size, n, device=0):
        _Block.__init__(self)
        self._item = int(item_size)
        self._create(self._item, int(n), int(device))

    def set_n(self, n):
        self._call("set_n", int(n))

    def produced(self, n_in):
        return self._call("produced", int(n_in))

    def work(self, n_in, input_items):
        x = np.ascontiguousarray(input_items)
        raw = x.reshape(-1).view(np.uint8)
        if len(raw) < n_in * self._streams * self._item:
            raise ValueError("work needs %d input bytes, got %d" % (n_in * self._streams * self._item, len(raw)))
        out = np.zeros(max(self.produced(n_in), 1) * self._streams * self._item, dtype=np.uint8)
        r = self._call("work", int(n_in), _ptr(raw), _ptr(out))
        out = out[:r * self._streams * self._item]
        return out.view(x.dtype) if self._item % x.dtype.itemsize == 0 else out


# ----------------------------------------------------------------------------
# blks2.logpwrfft_c / logpwrfft_f (blks2impl/logpwrfft.py:26-154) and window.blackmanharris (gnuradio/window.py:166-176)
# ----------------------------------------------------------------------------
def window_blackmanharris(fft_size):
    """window.blackmanharris(fft_size): the doubles of the reference's closure; host arithmetic only, no device needed"""
    fft_size = int(fft_size)
    if fft_size < 0 or fft_size > (1 << 26):
        raise ValueError("fft_size out of range")
    out = np.zeros(max(fft_size, 1), dtype=np.float64)
    _check(lib().grhip_window_blackmanharris(fft_size, _ptr(out)))
    return out[:fft_size]


class _logpwrfft(_Block):
    """blks2.logpwrfft_X(sample_rate, fft_size, ref_scale, frame_rate, avg_alpha, average, win=None): win is the
    reference's window FUNCTION (called with fft_size) or the sequence of doubles it would return.  work takes whole
    frames of fft_size samples (streams back to back) and returns the kept frames' fft_size floats of dB each.
    set_streams restarts the averaging state and the frame countdown."""
    _in = None

    def __init__(self, sample_rate, fft_size, ref_scale, frame_rate, avg_alpha, average, win=None, device=0):
        _Block.__init__(self)
        self._n = int(fft_size)
        if callable(win):
            win = win(self._n)
        w = None if win is None else np.ascontiguousarray(win, dtype=np.float64).reshape(-1)
        self._create(float(sample_rate), self._n, float(ref_scale), float(frame_rate), float(avg_alpha),
                     int(bool(average)), None if w is None else _ptr(w), 0 if w is None else len(w), int(device))

    def set_decimation(self, decim):
        self._call("set_decimation", float(decim))

    def set_vec_rate(self, vec_rate):
        self._call("set_vec_rate", float(vec_rate))

    def set_sample_rate(self, sample_rate):
        self._call("set_sample_rate", float(sample_rate))

    def set_average(self, average):
        self._call("set_average", int(bool(average)))

    def set_avg_alpha(self, avg_alpha):
        self._call("set_avg_alpha", float(avg_alpha))

    def sample_rate(self):
        return self._fn("sample_rate")(self._h)

    def decimation(self):
        return self._call("decimation")

    def frame_rate(self):
        return self._fn("frame_rate")(self._h)

    def average(self):
        return bool(self._call("average"))

    def avg_alpha(self):
        return self._fn("avg_alpha")(self._h)

    def produced(self, n_frames):
        return self._call("produced", int(n_frames))

    def state(self):
        """the averaging filter's state: streams x fft_size floats of linear power"""
        out = np.zeros(self._streams * self._n, dtype=np.float32)
        self._call("state", _ptr(out))
        return out

    def work(self, n_frames, input_items):
        x = np.ascontiguousarray(input_items, dtype=self._in).reshape(-1)
        need = n_frames * self._streams * self._n
        if len(x) < need:
            raise ValueError("work needs %d input samples, got %d" % (need, len(x)))
        out = np.zeros(max(self.produced(n_frames), 1) * self._streams * self._n, dtype=np.float32)
        r = self._call("work", int(n_frames), _ptr(x), _ptr(out))
        return out[:r * self._streams * self._n]


class logpwrfft_c(_logpwrfft):
    _name = "logpwrfft_c"
    _in = np.complex64


class logpwrfft_f(_logpwrfft):
    _name = "logpwrfft_f"
    _in = np.float32


# ----------------------------------------------------------------------------
# gr.interp_fir_filter_XXX / gr.rational_resampler_base_XXX  (filter/gr_interp_fir_filter_XXX.i.t,
# filter/gr_rational_resampler_base_XXX.i.t) and blks2.rational_resampler_XXX
# (python/gnuradio/blks2impl/rational_resampler.py)
# ----------------------------------------------------------------------------
def _uint_arg(v):
    """a rate factor for a C unsigned: a negative one is out of range, as 0 is"""
    v = int(v)
    if v < 0:
        raise GrhipError(-2, "negative rate factor %d" % v)
    return v


class _rs_block(_Block):
    _kind = None
    _dtype = np.complex64
    _tap = np.float32

    def set_taps(self, taps):
        t = np.ascontiguousarray(taps, dtype=self._tap)
        self._call("set_taps", _ptr(t), len(t))

    def history(self):
        return self._call("history")

    def interpolation(self):
        return self._call("interpolation")

    def run_captures_device(self, n_streams, n_samples, d_in, in_stride_items, d_out, out_stride_items,
                            stream=None):
        """n_streams fresh captures in one launch; returns the outputs per capture.  d_out=None only returns that
        number."""
        n_out = C.c_size_t(0)
        self._call("run_captures_device", int(n_streams), int(n_samples), _devptr(d_in), int(in_stride_items),
                   _devptr(d_out), int(out_stride_items), C.byref(n_out), _stream(stream))
        return n_out.value

    def captures_nout(self, n_samples):
        """outputs of one fresh capture of n_samples items"""
        return self.run_captures_device(1, n_samples, None, n_samples, None, 0)


class _interp_fir_filter(_rs_block):
    _name = "interp_fir_filter"

    def __init__(self, interpolation, taps, device=0):
        _Block.__init__(self)
        t = np.ascontiguousarray(taps, dtype=self._tap)
        self._create(self._kind.encode(), _uint_arg(interpolation), _ptr(t), len(t), int(device))

    def output_multiple(self):
        return self.interpolation()

    def work(self, noutput_items, input_items):
        """gr_sync_interpolator work: input_items carries history()-1 items in front and holds at least
        noutput_items/I + history() - 1; returns the outputs (none when the call installs latched taps)"""
        x = np.ascontiguousarray(input_items, dtype=self._dtype)
        n = int(noutput_items)
        I = self.interpolation()
        if n >= 0 and n % I == 0 and len(x) < n // I + self.history() - 1:
            raise ValueError("work: %d outputs need %d input items, got %d" % (n, n // I + self.history() - 1, len(x)))
        out = np.zeros(max(n, 1), dtype=self._dtype)
        r = self._call("work", n, _ptr(x), _ptr(out))
        return out[:r].copy()


class _rational_resampler_base(_rs_block):
    _name = "rational_resampler_base"

    def __init__(self, interpolation, decimation, taps, device=0):
        _Block.__init__(self)
        t = np.ascontiguousarray(taps, dtype=self._tap)
        self._create(self._kind.encode(), _uint_arg(interpolation), _uint_arg(decimation), _ptr(t), len(t),
                     int(device))

    def decimation(self):
        return self._call("decimation")

    def relative_rate(self):
        return 1.0 * self.interpolation() / self.decimation()

    def forecast(self, noutput_items):
        return self._call("forecast", int(noutput_items))

    def general_work(self, noutput_items, input_items):
        """returns (out, consumed); no history in front of input_items (the scheduler sees history 1)"""
        x = np.ascontiguousarray(input_items, dtype=self._dtype)
        out = np.zeros(max(int(noutput_items), 1), dtype=self._dtype)
        consumed = C.c_int(0)
        n = self._call("general_work", int(noutput_items), len(x), _ptr(x), _ptr(out), C.byref(consumed))
        return out[:n].copy(), consumed.value

    def general_work_device(self, noutput_items, ninput_items, d_in, d_out, stream=None):
        """returns (produced, consumed); the outputs are in d_out once `stream` has run"""
        consumed = C.c_int(0)
        n = self._call("general_work_device", int(noutput_items), int(ninput_items), _devptr(d_in), _devptr(d_out),
                       C.byref(consumed), _stream(stream))
        return n, consumed.value


class interp_fir_filter_ccf(_interp_fir_filter):
    """gr.interp_fir_filter_ccf(interpolation, taps)"""
    _kind = "ccf"


class interp_fir_filter_fff(_interp_fir_filter):
    """gr.interp_fir_filter_fff(interpolation, taps)"""
    _kind = "fff"
    _dtype = np.float32


class interp_fir_filter_ccc(_interp_fir_filter):
    """gr.interp_fir_filter_ccc(interpolation, taps)"""
    _kind = "ccc"
    _tap = np.complex64


class rational_resampler_base_ccf(_rational_resampler_base):
    """gr.rational_resampler_base_ccf(interpolation, decimation, taps)"""
    _kind = "ccf"


class rational_resampler_base_fff(_rational_resampler_base):
    """gr.rational_resampler_base_fff(interpolation, decimation, taps)"""
    _kind = "fff"
    _dtype = np.float32


class rational_resampler_base_ccc(_rational_resampler_base):
    """gr.rational_resampler_base_ccc(interpolation, decimation, taps)"""
    _kind = "ccc"
    _tap = np.complex64


def _izero(x):
    """Izero of general/gr_firdes.cc:35-49 (double)"""
    s = u = 1.0
    n = 1
    halfx = x / 2.0
    while True:
        temp = halfx / float(n)
        n += 1
        temp *= temp
        u *= temp
        s += u
        if not (u >= 1e-21 * s):
            return s


def _firdes_low_pass_kaiser(gain, sampling_freq, cutoff_freq, transition_width, beta):
    """gr_firdes::low_pass(..., WIN_KAISER, beta) of general/gr_firdes.cc:105-148, with compute_ntaps (:681-695) and
    3.5.0's one-sided Kaiser window (:759-772): float taps and window, the normalisation a double sum of the floats"""
    if sampling_freq <= 0.0:
        raise ValueError("gr_firdes check failed: sampling_freq > 0")
    if cutoff_freq <= 0.0 or cutoff_freq > sampling_freq / 2:
        raise ValueError("gr_firdes check failed: 0 < fa <= sampling_freq / 2")
    if transition_width <= 0:
        raise ValueError("gr_dirdes check failed: transition_width > 0")
    delta_f = transition_width / sampling_freq
    ntaps = int(10.0 / delta_f + 0.5)                  # width_factor[WIN_KAISER] = 10 (a float, exactly 10)
    if (ntaps & 1) == 0:
        ntaps += 1
    ibeta = 1.0 / _izero(beta)
    inm1 = 1.0 / float(ntaps)
    temp = np.arange(ntaps, dtype=np.float64) * inm1
    arg = beta * np.sqrt(1.0 - temp * temp)
    w = np.array([_izero(float(a)) * ibeta for a in arg], dtype=np.float32)
    M = (ntaps - 1) // 2
    fwT0 = 2 * np.pi * cutoff_freq / sampling_freq
    n = np.arange(-M, M + 1, dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        t = np.sin(n * fwT0) / (n * np.pi) * w.astype(np.float64)
    t[M] = fwT0 / np.pi * np.float64(w[M])
    taps = t.astype(np.float32)
    fmax = float(taps[M])
    for v in taps[M + 1:]:
        fmax += float(np.float32(2) * v)
    gain /= fmax
    return (taps.astype(np.float64) * gain).astype(np.float32)


def design_filter(interpolation, decimation, fractional_bw):
    """blks2impl/rational_resampler.py:26-56: low-pass taps of gain I at cutoff mid/I, transition tw/I, Kaiser beta 5"""
    if fractional_bw >= 0.5 or fractional_bw <= 0:
        raise ValueError("Invalid fractional_bandwidth, must be in (0, 0.5)")
    beta = 5.0
    trans_width = 0.5 - fractional_bw
    mid_transition_band = 0.5 - trans_width / 2
    return _firdes_low_pass_kaiser(interpolation, 1, mid_transition_band / interpolation,
                                   trans_width / interpolation, beta)


class _rational_resampler(object):
    """blks2impl/rational_resampler.py:60-100: the argument checks, I and D reduced by their gcd, taps designed when
    none are given (fractional_bw 0.4 when neither is), then a rational_resampler_base_XXX.  Its methods are the base
    block's (`resampler`)."""
    _base = None

    def __init__(self, interpolation, decimation, taps=None, fractional_bw=None, device=0):
        if not isinstance(interpolation, int) or interpolation < 1:
            raise ValueError("interpolation must be an integer >= 1")
        if not isinstance(decimation, int) or decimation < 1:
            raise ValueError("decimation must be an integer >= 1")
        if taps is None and fractional_bw is None:
            fractional_bw = 0.4
        d = math.gcd(interpolation, decimation)
        interpolation = interpolation // d
        decimation = decimation // d
        if taps is None:
            taps = design_filter(interpolation, decimation, fractional_bw)
        self.taps = np.asarray(taps)
        self.resampler = self._base(interpolation, decimation, taps, device)

    def __getattr__(self, name):
        return getattr(self.__dict__["resampler"], name)


class rational_resampler_ccf(_rational_resampler):
    """blks2.rational_resampler_ccf(interpolation, decimation, taps=None, fractional_bw=None)"""
    _base = rational_resampler_base_ccf


class rational_resampler_fff(_rational_resampler):
    """blks2.rational_resampler_fff(interpolation, decimation, taps=None, fractional_bw=None)"""
    _base = rational_resampler_base_fff


class rational_resampler_ccc(_rational_resampler):
    """blks2.rational_resampler_ccc(interpolation, decimation, taps=None, fractional_bw=None)"""
    _base = rational_resampler_base_ccc



# ----------------------------------------------------------------------------
# gr.pfb_interpolator_ccf / gr.pfb_synthesis_filterbank_ccf  (filter/gr_pfb_interpolator_ccf.i,
# filter/gr_pfb_synthesis_filterbank_ccf.i)
# ----------------------------------------------------------------------------
class pfb_interpolator_ccf(_interp_fir_filter):
    """gr.pfb_interpolator_ccf(interp, taps): gr_interp_fir_filter's schedule with the zeros behind the taps.
    (blks2.pfb_interpolator_ccf designs default taps with optfir; here the taps are required.)"""
    _name = "pfb_interpolator_ccf"

    def __init__(self, interp, taps, device=0):
        _Block.__init__(self)
        t = np.ascontiguousarray(taps, dtype=np.float32)
        self._create(_uint_arg(interp), _ptr(t), len(t), int(device))

    def taps_per_filter(self):
        return self.history()

    def run_captures_device(self, *args, **kwargs):
        raise NotImplementedError("pfb_interpolator_ccf has no run_captures_device entry; use work_device")

    def captures_nout(self, n_samples):
        raise NotImplementedError("pfb_interpolator_ccf has no run_captures_device entry; use work_device")


class pfb_synthesis_filterbank_ccf(_Block):
    """gr.pfb_synthesis_filterbank_ccf(numchans, taps): 1..numchans complex streams in, one stream out at numchans
    times the rate"""
    _name = "pfb_synthesis_filterbank_ccf"

    def __init__(self, numchans, taps, device=0):
        _Block.__init__(self)
        t = np.ascontiguousarray(taps, dtype=np.float32)
        self.numchans = int(numchans)
        self._create(_uint_arg(numchans), _ptr(t), len(t), int(device))

    def set_taps(self, taps):
        t = np.ascontiguousarray(taps, dtype=np.float32)
        self._call("set_taps", _ptr(t), len(t))

    def history(self):
        return self._call("history")

    def taps_per_filter(self):
        return self._call("taps_per_filter")

    def output_multiple(self):
        return self.numchans

    def work(self, noutput_items, streams):
        """gr_sync_interpolator work: streams is a list of 1..numchans complex arrays, each with history()-1 old items
        in front and at least noutput_items/numchans + history() - 1 items; returns the outputs (none when the call
        installs latched taps)"""
        arrs = [np.ascontiguousarray(s, dtype=np.complex64) for s in streams]
        n = int(noutput_items)
        M = self.numchans
        if n >= 0 and n % M == 0 and 1 <= len(arrs) <= M:
            need = n // M + self.history() - 1
            for a in arrs:
                if len(a) < need:
                    raise ValueError("work: %d outputs need %d items per stream, got %d" % (n, need, len(a)))
        ptrs = (C.c_void_p * max(len(arrs), 1))(*[a.ctypes.data for a in arrs])
        out = np.zeros(max(n, 1), dtype=np.complex64)
        r = self._call("work", n, ptrs, len(arrs), _ptr(out))
        return out[:r].copy()

    def work_device(self, noutput_items, d_in, stream_stride_items, numsigs, d_out, stream=None):
        """stream s at d_in + s*stream_stride_items; the outputs are in d_out once `stream` has run"""
        return self._call("work_device", int(noutput_items), _devptr(d_in), int(stream_stride_items), int(numsigs),
                          _devptr(d_out), _stream(stream))


# ----------------------------------------------------------------------------
# full DMR chain (multi-stream, device resident)
# ----------------------------------------------------------------------------
class _ChainParams(C.Structure):
    _fields_ = [("decimation", C.c_int), ("taps", C.c_void_p), ("ntaps", C.c_size_t),
                ("center_freq", C.c_double), ("sampling_freq", C.c_double), ("demod_gain", C.c_float),
                ("omega", C.c_float), ("gain_omega", C.c_float), ("mu", C.c_float), ("gain_mu", C.c_float),
                ("omega_relative_limit", C.c_float), ("access_code", C.c_char_p),
                ("access_code_len", C.c_size_t), ("threshold", C.c_int)]


class dmr_chain(_Block):
    _name = "dmr_chain"

    def __init__(self, decimation, taps, center_freq, sampling_freq, demod_gain, omega, gain_omega, mu,
                 gain_mu, omega_relative_limit, access_code, threshold, n_streams, max_samples, device=0):
        _Block.__init__(self)
        self._taps = np.ascontiguousarray(taps, dtype=np.complex64)
        code = access_code.encode("latin-1") if isinstance(access_code, str) else bytes(access_code)
        self._code = code
        p = _ChainParams(int(decimation), self._taps.ctypes.data, len(self._taps), float(center_freq),
                         float(sampling_freq), float(demod_gain), float(omega), float(gain_omega), float(mu),
                         float(gain_mu), float(omega_relative_limit), code, len(code), int(threshold))
        self.n_streams = int(n_streams)
        self._create(C.byref(p), self.n_streams, int(max_samples), int(device))

    def set_captures_per_wave(self, captures):
        self._call("set_captures_per_wave", int(captures))

    def set_max_symbols(self, max_symbols):
        """noutput_items of the clock recovery per capture (0: unbounded)"""
        self._call("set_max_symbols", int(max_symbols))

    def set_four_level(self, enable, pager_alpha=0.001):
        """4FSK tail: pager.slicer_fb(alpha) -> unpack_k_bits_bb(2) -> correlator; two output items per symbol"""
        self._call("set_four_level", int(bool(enable)), float(pager_alpha))

    def run_device(self, d_in, n_samples, stream_stride_items, d_bits, bits_stride, d_nbits, stream=None):
        return self._call("run_device", _devptr(d_in), int(n_samples), int(stream_stride_items), _devptr(d_bits),
                          int(bits_stride), _devptr(d_nbits), _stream(stream))

    def intermediate(self, which):
        p = C.c_void_p(0)
        stride = C.c_size_t(0)
        self._call("intermediate", int(which), C.byref(p), C.byref(stride))
        return p.value, stride.value


# ----------------------------------------------------------------------------
# minimal stand-in for the scheduler around ONE sync block / decimator:
# history-1 zeros preloaded (runtime/gr_flat_flowgraph.cc:150), then work() in
# chunks of at most `chunk` outputs (runtime/gr_block_executor.cc:76-78 caps a
# call at half a 64 KiB buffer), re-presenting the history in front of each call
# (runtime/gr_sync_decimator.cc:46-66).  A work() that returns 0 items (taps
# update) is simply called again, as the executor would.
# ----------------------------------------------------------------------------
def run_sync_block(block, x, chunk=4096, out_dtype=None):
    h = block.history()
    d = block.decimation()
    buf = np.concatenate([np.zeros(h - 1, dtype=x.dtype), x])
    n_total = len(x) // d
    outs = []
    done = 0
    retries = 0
    while done < n_total:
        n = min(chunk, n_total - done)
        seg = buf[done * d: done * d + n * d + h - 1]
        y = block.work(n, seg)
        if len(y) == 0:
            # history may have changed
            retries += 1
            if retries > 4:
                raise RuntimeError("block keeps returning 0 items")
            nh = block.history()
            if nh != h:
                # re-present with the new history length: keep alignment of the
                # newest item, like the scheduler's read pointer does
                x_pos = done * d
                raw = np.concatenate([np.zeros(nh - 1, dtype=x.dtype), x])
                buf = raw
                h = nh
                _ = x_pos
            continue
        outs.append(y)
        done += len(y)
    if not outs:
        return np.zeros(0, dtype=out_dtype or x.dtype)
    return np.concatenate(outs)
