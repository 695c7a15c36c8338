"""ctypes binding of libx3hip.so (include/x3hip.h): the MI355X-native X3 encoder/decoder.

Thin by design: every call goes straight to the C ABI, which runs the HIP kernels.  There is
no Python or CPU implementation behind it -- if the library or a GPU is missing, loading or
context creation raises.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(os.path.dirname(_HERE), "lib", "libx3hip.so")
if os.environ.get("X3HIP_LIB"):   # (development: an experiment build of the same library, tools/variants.py)
    LIB_PATH = os.environ["X3HIP_LIB"]

OK = 0
ERR_INVALID_ENCODING_THRESH = 4
ERR_OUT_OF_BOUNDS_INVERSE = 5
ERR_MORE_THAN_ONE_CHANNEL = 6
ERR_FRAME_LENGTH = 10
ERR_FRAME_HEADER_INVALID_KEY = 11
ERR_FRAME_HEADER_INVALID_PAYLOAD_LEN = 12
ERR_FRAME_HEADER_INVALID_HEADER_CRC = 13
ERR_FRAME_HEADER_INVALID_PAYLOAD_CRC = 14
ERR_FRAME_DECODE_INVALID_BPF = 20
ERR_FRAME_DECODE_UNEXPECTED_END = 21
ERR_BYTE_WRITER_INSUFFICIENT_MEMORY = 22
ERR_HIP = 23
ERR_BAD_ARG = 24

# every symbol include/x3hip.h declares (tests check that the library exports all of them)
SYMBOLS = [
    "x3_strerror", "x3_ctx_create", "x3_ctx_create_on_stream", "x3_ctx_destroy", "x3_ctx_sync", "x3_last_error",
    "x3_ctx_set_option", "x3_ctx_get_option",
    "x3_ctx_enable_kernel_timing", "x3_ctx_kernel_time", "x3_ctx_kernel_times", "x3_ctx_launch_log", "x3_ctx_reset_kernel_time",
    "x3_params_default", "x3_params_validate", "x3_rice_code_get", "x3_num_frames", "x3_encode_bound",
    "x3_crc16", "x3_crc16_dev", "x3_crc16_update",
    "x3_encode", "x3_encode_frame", "x3_write_frame_header", "x3_encode_batch",
    "x3_read_frame_header", "x3_decode_frame", "x3_decode_prefetch", "x3_decode_stream",
    "x3_archive_header_write", "x3_archive_header_read", "x3_x3a_encode", "x3_x3a_decode",
    "x3_wav_to_x3a", "x3_x3a_to_wav",
    "x3_bitreader_new", "x3_bitreader_read_nbits", "x3_bitreader_count_zero_bits", "x3_bitreader_inc_bits",
    "x3_bitreader_state", "x3_bitreader_free", "x3_decode_block",
    "x3_bitpacker_new", "x3_bitpacker_write_bits", "x3_bitpacker_write_packed_zeros", "x3_bitpacker_write_bytes", "x3_bitpacker_inc_counter_n_bytes", "x3_bitpacker_word_align",
    "x3_bitpacker_finish", "x3_bitpacker_peek", "x3_bitpacker_take", "x3_bitpacker_free",
    "x3_reader_open", "x3_reader_open_mem", "x3_reader_spec", "x3_reader_next_frame", "x3_reader_frame_errors",
    "x3_reader_position", "x3_reader_close",
    "x3_encode_dev", "x3_encode_frames_dev", "x3_encode_result", "x3_decode_dev", "x3_decode_result", "x3_index_dev", "x3_decode_stream_dev",
    "x3_seg_index_entries", "x3_decode_dev_seg", "x3_encode_dev_seg", "x3_seg_index_build_dev", "x3_place_buffers",
    "x3_graph_begin", "x3_graph_end", "x3_graph_launch", "x3_graph_destroy",
    "x3_synth", "x3_synth_dev", "x3_dev_alloc", "x3_dev_free", "x3_dev_upload", "x3_dev_download",
    "x3_shard_unique_id", "x3_shard_create", "x3_shard_destroy", "x3_shard_rank", "x3_shard_world",
    "x3_shard_frame_range", "x3_shard_sample_range", "x3_shard_offsets", "x3_shard_exchange_lengths",
    "x3_shard_exchange_length_value", "x3_shard_lengths", "x3_shard_gather", "x3_shard_gather_async", "x3_shard_gather_wait", "x3_shard_write_at",
    "x3_mgpu_create", "x3_mgpu_destroy", "x3_mgpu_devices", "x3_mgpu_ctx", "x3_mgpu_shard", "x3_mgpu_last_error",
    "x3_mgpu_encode", "x3_mgpu_decode_stream",
    "x3_encode_mc", "x3_decode_stream_mc",
    "x3_sample_offsets_dev", "x3_decode_windows_dev", "x3_decode_windows_result",
    "x3_decode_ranges_dev", "x3_corpus_ranges_dev", "x3_decode_ranges_result",
    "x3_decode_streams_dev", "x3_decode_streams_result",
    "x3_corpus_build", "x3_corpus_info", "x3_corpus_entries", "x3_corpus_entries_dev", "x3_corpus_seg_index", "x3_corpus_windows_dev",
    "x3_corpus_destroy",
    "x3_levels_dev", "x3_levels_result", "x3_corpus_levels_rows", "x3_corpus_levels_dev",
    "x3_signal_levels_dev", "x3_corpus_signal_levels_dev", "x3_fir_levels_dev", "x3_corpus_fir_levels_dev",
    "x3_tone_levels_dev", "x3_corpus_tone_levels_dev", "x3_tone_power_levels_dev",
    "x3_tone_bank_levels_dev", "x3_corpus_tone_bank_levels_dev",
    "x3_events_dev", "x3_corpus_events_dev", "x3_events_result",
    "x3_level_quantiles_dev", "x3_corpus_level_quantiles_dev", "x3_level_quantiles_result",
    "x3_level_thresholds_dev", "x3_corpus_level_thresholds_dev", "x3_events_adaptive_dev", "x3_corpus_events_adaptive_dev",
    "x3_plane_events_dev", "x3_corpus_plane_events_dev",
    "x3_range_levels_dev", "x3_corpus_range_levels_dev", "x3_range_levels_result",
    "x3_signal_range_levels_dev", "x3_corpus_signal_range_levels_dev",
    "x3_fir_range_levels_dev", "x3_corpus_fir_range_levels_dev",
    "x3_tone_range_levels_dev", "x3_corpus_tone_range_levels_dev",
    "x3_tone_bank_range_levels_dev", "x3_corpus_tone_bank_range_levels_dev",
    "x3_spectra_rows_dev", "x3_spectra_result", "x3_spectra_levels_dev",
    "x3_tune_candidate", "x3_tuner_create", "x3_tuner_add_dev", "x3_tuner_result", "x3_tuner_max_payloads",
    "x3_tuner_reset", "x3_tuner_destroy", "x3_tune", "x3_x3a_encode_tuned",
]

TUNE_CANDIDATES, TUNE_DEFAULT_INDEX, TUNE_DEFAULT_SPF = 2184, 1188, 10000   # include/x3hip.h, "parameter tuning"

WINDOW_I16, WINDOW_F32 = 0, 1   # x3_decode_windows_dev output formats
STREAMS_ARCHIVE_FRAMES = 1       # x3_decode_streams_dev: entries are the frame part of .x3a archives
CORPUS_INDEX_WALK = 0x100        # x3_corpus_build: the segment index by x3_seg_index_build_dev (any parameters)
LEVEL_SIGNAL_SAMPLES, LEVEL_SIGNAL_DIFF = 0, 1   # x3_signal_levels_dev: the samples, or their clamped first difference
LEVEL_SIGNALS = {"samples": LEVEL_SIGNAL_SAMPLES, "diff": LEVEL_SIGNAL_DIFF}   # the mirrors' keyword `signal`


class LevelFir(C.Structure):
    """x3_level_fir: the taps and shift of x3_fir_levels_dev / x3_corpus_fir_levels_dev"""
    _fields_ = [("n_taps", C.c_uint32), ("shift", C.c_uint32), ("taps", C.c_int16 * 8)]


class Fir:
    """An integer FIR filter in front of the levels: y[i] = clamp((sum over t of taps[t] * x[i - t]) >> shift, 16 bits),
    counted where all len(taps) positions lie in good frames of the same stream or entry (x3_fir_levels_dev).  1 .. 8 taps
    of 16 bits with sum |taps| <= 32768, shift 0 .. 15; immutable, checked here.  Goes wherever `signal=` goes."""
    __slots__ = ("taps", "shift")

    def __init__(self, taps, shift=0):
        t = tuple(int(c) for c in taps)
        if any(isinstance(c, bool) or int(c) != c for c in taps) or isinstance(shift, bool) or int(shift) != shift:
            raise ValueError("Fir: integer taps and shift")
        if not 1 <= len(t) <= 8:
            raise ValueError("Fir: 1 .. 8 taps")
        if not 0 <= int(shift) <= 15:
            raise ValueError("Fir: shift 0 .. 15")
        if any(not -32768 <= c <= 32767 for c in t) or sum(abs(c) for c in t) > 32768:
            raise ValueError("Fir: taps of 16 bits with sum |taps| <= 32768")
        object.__setattr__(self, "taps", t)
        object.__setattr__(self, "shift", int(shift))

    def __setattr__(self, name, value):
        raise AttributeError("Fir is immutable")

    __delattr__ = __setattr__

    def __eq__(self, other):
        return isinstance(other, Fir) and (self.taps, self.shift) == (other.taps, other.shift)

    def __hash__(self):
        return hash((self.taps, self.shift))

    def __repr__(self):
        return "Fir(%r, shift=%d)" % (list(self.taps), self.shift)

    def c_struct(self):
        """-> the x3_level_fir of this filter"""
        return LevelFir(len(self.taps), self.shift, (C.c_int16 * 8)(*self.taps))


class LevelTone(C.Structure):
    """x3_level_tone: the oscillator of x3_tone_levels_dev / x3_corpus_tone_levels_dev; d_table is a device pointer"""
    _fields_ = [("step", C.c_uint32), ("reserved", C.c_uint32), ("d_table", C.c_void_p)]


TONE_BANK_MAX = 8   # X3_TONE_BANK_MAX: the oscillators of one tone bank call


class LevelToneBank(C.Structure):
    """x3_level_tone_bank: the oscillators of x3_tone_bank_levels_dev / x3_corpus_tone_bank_levels_dev against one table;
    d_table is a device pointer, steps behind n_tones are never read"""
    _fields_ = [("n_tones", C.c_uint32), ("reserved", C.c_uint32), ("d_table", C.c_void_p),
                ("steps", C.c_uint32 * TONE_BANK_MAX)]


TONE_TABLE_PAIRS = 1024   # (cos, sin) int16 pairs of a tone table: 4 096 bytes

SPECTRA_SUMS, SPECTRA_POWER = 0, 1   # X3_SPECTRA_*: rows of (re, im) int64 pairs / of uint32 band powers
SPECTRA_NFFTS = (64, 128, 256, 512, 1024)


class SpectraRule(C.Structure):
    """x3_spectra_rule: the transform of x3_spectra_rows_dev -- n_fft in SPECTRA_NFFTS, hop >= 1, format SPECTRA_SUMS or
    SPECTRA_POWER, reserved 0; d_table is a device pointer to a tone table (24 bytes, copied at the call)"""
    _fields_ = [("n_fft", C.c_uint32), ("hop", C.c_uint32), ("format", C.c_uint32), ("reserved", C.c_uint32),
                ("d_table", C.c_void_p)]


class SpectraFold(C.Structure):
    """x3_spectra_fold: how x3_spectra_levels_dev folds the POWER words -- frames_per_bin consecutive frames into a time bin,
    the bins k of a frame into band d_bin_band[k] (a device pointer to n_fft / 2 + 1 uint32 words; a word >= n_bands: no
    band), plane b of the records at b * plane_stride records (0: rows_cap), reserved 0 (32 bytes, copied at the call)"""
    _fields_ = [("frames_per_bin", C.c_uint32), ("n_bands", C.c_uint32), ("plane_stride", C.c_uint64),
                ("d_bin_band", C.c_void_p), ("reserved", C.c_uint64)]


def band_edges_third_octave(n_fft, sample_rate, f_lo, f_hi):
    """The bin edges of the third-octave bands (base two: centre frequencies 1 000 * 2^(i / 3) Hz, a band from
    fc * 2^(-1/6) to fc * 2^(1/6)) whose centres lie in [f_lo, f_hi], for range_band_levels(bands=...) -> a list of K + 1
    ascending ints: band b holds the bins [edges[b], edges[b + 1]) of n_fft / 2 + 1, bin k at k * sample_rate / n_fft Hz
    and counted to the band that holds its centre frequency.  A band narrower than a bin holds no bin; a ValueError when
    no centre lies in the interval or below sample_rate / 2."""
    import math
    nb, df = n_fft // 2 + 1, float(sample_rate) / n_fft
    if not 0 < f_lo <= f_hi:
        raise ValueError("0 < f_lo <= f_hi")
    i0, i1 = math.ceil(3 * math.log2(f_lo / 1000.0) - 1e-9), math.floor(3 * math.log2(f_hi / 1000.0) + 1e-9)
    cuts = [1000.0 * 2.0 ** ((2 * i - 1) / 6.0) for i in range(i0, i1 + 2)]    # lower edge of band i; the last: the upper of i1
    edges = [min(nb, max(0, math.ceil(c / df - 1e-9))) for c in cuts]
    while len(edges) > 1 and edges[-2] >= nb:                                  # (bands wholly above the last bin)
        edges.pop()
    if len(edges) < 2:
        raise ValueError("no third-octave centre in [f_lo, f_hi] below sample_rate / 2")
    return edges


def spectra_bin_band(n_fft, bands):
    """bands of range_band_levels -> (bin_band np.uint32 [n_fft / 2 + 1], K).  None: one band per bin.  A torch tensor or
    numpy array of exactly n_fft / 2 + 1 integers: the band of every bin as it is (any word, as the library takes them),
    K = the largest index below n_fft / 2 + 1, plus one.  Any other sequence: K + 1 ascending bin edges, band b the bins
    [edges[b], edges[b + 1]), every other bin in no band."""
    nb = n_fft // 2 + 1
    if bands is None:
        return np.arange(nb, dtype=np.uint32), nb
    is_array = hasattr(bands, "cpu") or isinstance(bands, np.ndarray)
    a = np.asarray(bands.cpu().numpy() if hasattr(bands, "cpu") else bands)
    if a.ndim != 1 or a.dtype.kind not in "iu":
        raise ValueError("bands: K + 1 ascending bin edges, or an array of n_fft / 2 + 1 band indices")
    if is_array and a.size == nb:
        m = a.astype(np.int64) & 0xFFFFFFFF
        inside = m[m < nb]
        if inside.size == 0:
            raise ValueError("bands: no bin in any band")
        return m.astype(np.uint32), int(inside.max()) + 1
    e = a.astype(np.int64)
    if e.size < 2 or e.size - 1 > nb or (np.diff(e) < 0).any() or e[0] < 0 or e[-1] > nb:
        raise ValueError("bands: K + 1 ascending bin edges in 0 .. n_fft / 2 + 1, K in 1 .. n_fft / 2 + 1")
    m = np.full(nb, 0xFFFFFFFF, dtype=np.uint32)
    for b in range(e.size - 1):
        m[e[b]:e[b + 1]] = b
    return m, e.size - 1


def spectra_n_rows(length, n_fft, hop):
    """R of a row of `length` samples: whole frames only"""
    return 0 if length < n_fft else (length - n_fft) // hop + 1


def tone_table():
    """-> the usual table, np.int16 [1024, 2]: (round(32767 cos(2 pi k / 1024)), round(32767 sin(2 pi k / 1024))) at pair k"""
    a = 2.0 * np.pi * np.arange(TONE_TABLE_PAIRS) / TONE_TABLE_PAIRS
    return np.stack([np.rint(32767.0 * np.cos(a)), np.rint(32767.0 * np.sin(a))], axis=1).astype(np.int16)


class Tone:
    """One oscillator in front of the levels: position i has the phase (i * step) mod 2^32, and a bin's record holds the
    quadrature sums of its samples against the usual table (tone_table(); x3_tone_levels_dev).  step: 0 .. 2^32 - 1, the
    frequency in units of sample_rate / 2^32; immutable, checked here.  tone_levels() returns the sums; wherever `signal=`
    goes a Tone means those sums through tone_power_levels_dev: the level records of the band."""
    __slots__ = ("step",)

    def __init__(self, step):
        if isinstance(step, bool) or not isinstance(step, (int, np.integer)) or not 0 <= int(step) <= 0xFFFFFFFF:
            raise ValueError("Tone: an integer step, 0 .. 2^32 - 1")
        object.__setattr__(self, "step", int(step))

    @classmethod
    def at(cls, freq, sample_rate):
        """the Tone nearest to `freq` at `sample_rate` (0 <= freq < sample_rate): step = round(freq / sample_rate * 2^32),
        and 2^32 - 1, the last step below the sample rate, where that rounds to 2^32 (which would be step 0: DC)"""
        if not sample_rate > 0 or not 0 <= freq < sample_rate:
            raise ValueError("Tone.at: 0 <= freq < sample_rate")
        return cls(min(int(round(float(freq) / float(sample_rate) * 4294967296.0)), 0xFFFFFFFF))

    @classmethod
    def bank(cls, freqs, sample_rate):
        """-> the tuple of Tone.at(f, sample_rate) for f in freqs: the `tones` of tone_bank_levels (1 .. TONE_BANK_MAX)"""
        return tuple(cls.at(f, sample_rate) for f in freqs)

    def __setattr__(self, name, value):
        raise AttributeError("Tone is immutable")

    def __delattr__(self, name):
        raise AttributeError("Tone is immutable")

    def __eq__(self, other):
        return isinstance(other, Tone) and self.step == other.step

    def __hash__(self):
        return hash(("Tone", self.step))

    def __repr__(self):
        return "Tone(step=%d)" % self.step


def tone_bank(tones):
    """the `tones` of the tone bank calls -> a tuple of 1 .. TONE_BANK_MAX Tone, or ValueError"""
    if isinstance(tones, Tone):
        raise ValueError("tones: a sequence of 1 .. %d Tone (one Tone: tone_levels)" % TONE_BANK_MAX)
    try:
        tones = tuple(tones)
    except TypeError:
        raise ValueError("tones: a sequence of 1 .. %d Tone" % TONE_BANK_MAX) from None
    if not 1 <= len(tones) <= TONE_BANK_MAX or not all(isinstance(t, Tone) for t in tones):
        raise ValueError("tones: a sequence of 1 .. %d Tone" % TONE_BANK_MAX)
    return tones


def level_signal(signal, fir=True):
    """the keyword `signal` of the levels methods ("samples" | "diff", or a LEVEL_SIGNAL_* value) -> the C ABI's int; a
    Fir or a Tone is handed through (fir=False: to the range-levels keyword, which takes neither and raises;
    fir_range_levels and tone_range_levels do, and tone_bank_range_levels takes a bank of Tones)"""
    if not fir and isinstance(signal, (tuple, list, LevelToneBank)):
        raise ValueError("signal: range levels of a tone bank are not built on this keyword: call tone_bank_range_levels")
    if isinstance(signal, Fir):
        if not fir:
            raise ValueError("signal: range levels of a Fir signal are not built yet on this keyword: call fir_range_levels")
        return signal
    if isinstance(signal, Tone):
        if not fir:
            raise ValueError("signal: range levels of a Tone signal are not built yet on this keyword: call tone_range_levels")
        return signal
    if signal in LEVEL_SIGNALS:
        return LEVEL_SIGNALS[signal]
    if signal in LEVEL_SIGNALS.values() and not isinstance(signal, bool):
        return int(signal)
    raise ValueError('signal: "samples", "diff", a Fir or a Tone')


# x3_tone_level: one bin of x3_tone_levels_dev / x3_corpus_tone_levels_dev (32 bytes, x3_level's layout slot for slot)
TONE_DTYPE = np.dtype([("re", np.int64), ("im", np.int64), ("min", np.int32), ("max", np.int32), ("n", np.uint32),
                       ("reserved", np.uint32)])
# x3_level: one bin of x3_levels_dev / x3_corpus_levels_dev (32 bytes)
LEVEL_DTYPE = np.dtype([("sum_sq", np.uint64), ("sum", np.int64), ("min", np.int32), ("max", np.int32), ("n", np.uint32),
                        ("reserved", np.uint32)])


class EventRule(C.Structure):
    """x3_event_rule: which bins of level records are hot and how runs of them become events (x3_events_dev)"""
    _fields_ = [("mean_sq_min", C.c_uint64), ("peak_min", C.c_uint32), ("join_bins", C.c_uint32), ("min_bins", C.c_uint32),
                ("pad_bins", C.c_uint32), ("max_bins", C.c_uint32), ("reserved", C.c_uint32)]

    @classmethod
    def make(cls, mean_sq_min=0, peak_min=0, join_bins=0, min_bins=0, pad_bins=0, max_bins=0):
        return cls(mean_sq_min, peak_min, join_bins, min_bins, pad_bins, max_bins, 0)


EVENT_RULE_DTYPE = np.dtype([("mean_sq_min", "<u8"), ("peak_min", "<u4"), ("join_bins", "<u4"), ("min_bins", "<u4"),
                             ("pad_bins", "<u4"), ("max_bins", "<u4"), ("reserved", "<u4")])


EVENT_PLANES_MAX = 8   # X3_EVENT_PLANES_MAX: the planes of one plane events call


class PlaneEventRule(C.Structure):
    """x3_plane_event_rule: a row is hot when at least min_planes of n_planes planes are loud at it, each plane under its own
    two values; join_bins, min_bins, pad_bins and max_bins are EventRule's (x3_plane_events_dev)"""
    _fields_ = [("n_planes", C.c_uint32), ("min_planes", C.c_uint32), ("join_bins", C.c_uint32), ("min_bins", C.c_uint32),
                ("pad_bins", C.c_uint32), ("max_bins", C.c_uint32), ("reserved", C.c_uint32 * 2),
                ("mean_sq_min", C.c_uint64 * EVENT_PLANES_MAX), ("peak_min", C.c_uint32 * EVENT_PLANES_MAX)]

    @classmethod
    def make(cls, mean_sq_min=None, peak_min=None, min_planes=1, join_bins=0, min_bins=0, pad_bins=0, max_bins=0, n_planes=None):
        """mean_sq_min, peak_min: a value per plane (one of them may be left out: all 0); n_planes: their length unless
        given, which a rule for thresholds per entry needs (no values at all)"""
        ms, pk = list(mean_sq_min or []), list(peak_min or [])
        k = max(len(ms), len(pk)) if n_planes is None else int(n_planes)
        if not 1 <= k <= EVENT_PLANES_MAX or len(ms) not in (0, k) or len(pk) not in (0, k):
            raise ValueError("1 .. %d planes, a value per plane" % EVENT_PLANES_MAX)
        r = cls(k, min_planes, join_bins, min_bins, pad_bins, max_bins)
        for t in range(k):
            r.mean_sq_min[t], r.peak_min[t] = (ms[t] if ms else 0), (pk[t] if pk else 0)
        return r


LEVEL_KEY_PEAK, LEVEL_KEY_MEAN_SQ = 0, 1   # x3_level_quantiles_dev: max(max, -min) / floor(sum_sq / n)


class ThresholdRule(C.Structure):
    """x3_threshold_rule: per criterion thr = clamp(floor(quantile(q_ppm) * mul / div) + add, 1, limit); div == 0: off"""
    _fields_ = [("peak_q_ppm", C.c_uint32), ("peak_mul", C.c_uint32), ("peak_div", C.c_uint32), ("peak_add", C.c_uint32),
                ("mean_sq_q_ppm", C.c_uint32), ("mean_sq_mul", C.c_uint32), ("mean_sq_div", C.c_uint32),
                ("mean_sq_add", C.c_uint32)]

    @classmethod
    def make(cls, peak=None, mean_sq=None):
        """peak / mean_sq: (q_ppm, mul, div, add) or None for a criterion that is off"""
        return cls(*(tuple(peak or (0, 0, 0, 0)) + tuple(mean_sq or (0, 0, 0, 0))))


# x3_event_threshold: the two values of the events rule for one entry, and its counting rows (16 bytes)
EVENT_THRESHOLD_DTYPE = np.dtype([("mean_sq_min", "<u8"), ("peak_min", "<u4"), ("counted", "<u4")])


def event_levels_view(t):
    """the merged records of events() / a [n, 32] uint8 tensor or array of x3_level records -> np.ndarray of LEVEL_DTYPE [n]"""
    a = t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)
    return np.ascontiguousarray(a).view(np.uint8).reshape(-1).view(LEVEL_DTYPE)


class StreamResult(C.Structure):
    """x3_stream_result: one entry of x3_decode_streams_dev"""
    _fields_ = [("n_out", C.c_uint64), ("frames_ok", C.c_uint64), ("status", C.c_int32), ("frame_errors", C.c_uint32)]


STREAM_RESULT_DTYPE = np.dtype([("n_out", "<u8"), ("frames_ok", "<u8"), ("status", "<i4"), ("frame_errors", "<u4")])
# x3_corpus_entry: one entry of a Corpus
CORPUS_ENTRY_DTYPE = np.dtype([("n_samples", "<u8"), ("first_frame", "<u8"), ("n_frames", "<u8"), ("walk_status", "<i4"),
                               ("general_walk", "<u4")])


class RiceCode(C.Structure):
    """x3_rice_code (RiceCode, src/x3.rs:187-194)"""
    _fields_ = [("nsubs", C.c_uint32), ("offset", C.c_uint32), ("len", C.c_uint32), ("inv_len", C.c_uint32),
                ("code", C.POINTER(C.c_uint32)), ("num_bits", C.POINTER(C.c_uint32)), ("inv", C.POINTER(C.c_int16))]


class Params(C.Structure):
    """x3::Parameters (src/x3.rs:81-134)"""
    _fields_ = [("block_len", C.c_uint32), ("blocks_per_frame", C.c_uint32),
                ("codes", C.c_uint32 * 3), ("thresholds", C.c_uint32 * 3)]

    @classmethod
    def default(cls):
        p = cls()
        lib().x3_params_default(C.byref(p))
        return p

    @classmethod
    def make(cls, block_len=20, blocks_per_frame=500, codes=(0, 1, 3), thresholds=(3, 8, 20)):
        return cls(block_len, blocks_per_frame, (C.c_uint32 * 3)(*codes), (C.c_uint32 * 3)(*thresholds))

    @property
    def spf(self):
        return self.block_len * self.blocks_per_frame


class FrameHeader(C.Structure):
    """x3::FrameHeader (src/x3.rs:148-184)"""
    _fields_ = [("source_id", C.c_uint8), ("channels", C.c_uint8), ("samples", C.c_uint16),
                ("payload_len", C.c_uint32), ("payload_crc", C.c_uint16)]


class Batch(C.Structure):
    _fields_ = [("n_per_clip", C.c_uint64), ("clip_stride", C.c_uint64), ("n_clips", C.c_uint64)]


_lib = None


def _preload_torch_hip_runtime():
    """PyTorch wheels bundle their own libamdhip64.so (same SONAME as /opt/rocm's).  Two HIP
    runtimes in one process cannot both own the GPU, so when torch is installed its copy is loaded
    first and libx3hip.so's DT_NEEDED libamdhip64.so.7 then binds to it -- in either import order
    bench.py (torch for HBM tensors / streams / RCCL + this library for the kernels) sees one runtime.
    Without torch the system runtime from /opt/rocm is used."""
    if os.environ.get("X3HIP_SYSTEM_HIP") == "1":
        return
    try:
        import importlib.util
        spec = importlib.util.find_spec("torch")
        if spec is None or not spec.submodule_search_locations:
            return
        cand = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
        if os.path.exists(cand):
            C.CDLL(cand, mode=C.RTLD_GLOBAL)
    except Exception:
        pass


def lib():
    """Load libx3hip.so; raises if it has not been built (python x3-rust_amd/build.py)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError("libx3hip.so is missing (%s): run `python x3-rust_amd/build.py`; "
                           "there is no CPU fallback" % LIB_PATH)
    _preload_torch_hip_runtime()
    L = C.CDLL(LIB_PATH)
    vp, u64, u32, i32 = C.c_void_p, C.c_uint64, C.c_uint32, C.c_int
    PP = C.POINTER(Params)
    L.x3_strerror.restype = C.c_char_p
    L.x3_strerror.argtypes = [i32]
    L.x3_ctx_create.argtypes = [i32, C.POINTER(vp)]
    L.x3_ctx_create_on_stream.argtypes = [i32, vp, C.POINTER(vp)]
    L.x3_ctx_destroy.restype = None
    L.x3_ctx_destroy.argtypes = [vp]
    L.x3_ctx_sync.argtypes = [vp]
    L.x3_last_error.restype = C.c_char_p
    L.x3_last_error.argtypes = [vp]
    L.x3_ctx_set_option.argtypes = [vp, C.c_char_p, C.c_longlong]
    L.x3_ctx_get_option.argtypes = [vp, C.c_char_p, C.POINTER(C.c_longlong)]
    L.x3_ctx_enable_kernel_timing.argtypes = [vp, i32]
    L.x3_ctx_kernel_time.argtypes = [vp, i32, C.POINTER(C.c_double), C.POINTER(u64)]
    L.x3_ctx_kernel_times.argtypes = [vp, i32, C.POINTER(C.c_double), u64, C.POINTER(u64)]
    L.x3_ctx_launch_log.argtypes = [vp, i32, C.POINTER(C.c_uint32), u64, C.POINTER(u64)]
    L.x3_ctx_reset_kernel_time.argtypes = [vp]
    L.x3_params_default.restype = None
    L.x3_params_default.argtypes = [PP]
    L.x3_params_validate.argtypes = [PP]
    L.x3_rice_code_get.argtypes = [C.c_uint32, C.POINTER(RiceCode)]
    L.x3_num_frames.restype = u64
    L.x3_num_frames.argtypes = [u64, PP]
    L.x3_encode_bound.restype = u64
    L.x3_encode_bound.argtypes = [u64, PP]
    L.x3_crc16.argtypes = [vp, vp, u64, C.POINTER(C.c_uint16)]
    L.x3_crc16_dev.argtypes = [vp, vp, u64, C.POINTER(C.c_uint16)]
    L.x3_crc16_update.restype = C.c_uint16
    L.x3_crc16_update.argtypes = [C.c_uint16, C.c_uint8]
    L.x3_encode.argtypes = [vp, vp, u64, u32, PP, vp, u64, u64, C.POINTER(u64), vp]
    L.x3_encode_frame.argtypes = [vp, vp, u64, PP, vp, u64, u64, C.POINTER(u64), vp]
    L.x3_write_frame_header.restype = None
    L.x3_write_frame_header.argtypes = [u64, C.c_uint8, u64, C.c_uint16, vp]
    L.x3_encode_batch.argtypes = [vp, C.POINTER(vp), C.POINTER(u64), u64, PP, vp, u64, C.POINTER(u64), vp]
    L.x3_read_frame_header.argtypes = [vp, u64, C.POINTER(FrameHeader)]
    L.x3_decode_frame.argtypes = [vp, vp, u64, vp, u64, PP, u64, C.POINTER(u64)]
    L.x3_decode_prefetch.argtypes = [vp, vp, u64, PP]
    L.x3_decode_stream.argtypes = [vp, vp, u64, PP, vp, u64, C.POINTER(u64), C.POINTER(u64), C.POINTER(u64)]
    L.x3_archive_header_write.argtypes = [u32, PP, vp, u64, C.POINTER(u64)]
    L.x3_archive_header_read.argtypes = [vp, u64, C.POINTER(u32), PP, C.POINTER(C.c_uint8), C.POINTER(u64)]
    L.x3_x3a_encode.argtypes = [vp, vp, u64, u32, vp, u64, C.POINTER(u64), vp]
    L.x3_x3a_decode.argtypes = [vp, vp, u64, vp, u64, C.POINTER(u64), C.POINTER(u32), C.POINTER(u64), C.POINTER(u64)]
    L.x3_wav_to_x3a.argtypes = [vp, C.c_char_p, C.c_char_p, vp]
    L.x3_x3a_to_wav.argtypes = [vp, C.c_char_p, C.c_char_p, C.POINTER(u64), C.POINTER(u64)]
    L.x3_encode_dev.argtypes = [vp, vp, C.POINTER(Batch), PP, vp, u64, u64, vp]
    L.x3_encode_frames_dev.argtypes = [vp, vp, vp, vp, u64, PP, vp, u64, u64, vp]
    L.x3_encode_result.argtypes = [vp, C.POINTER(u64), vp]
    L.x3_decode_dev.argtypes = [vp, vp, u64, vp, u64, C.POINTER(Batch), vp, PP, vp, u64, vp]
    L.x3_decode_result.argtypes = [vp, C.POINTER(u64), C.POINTER(i32), C.POINTER(u64)]
    L.x3_encode_dev_seg.argtypes = [vp, vp, C.POINTER(Batch), PP, vp, u64, u64, vp, vp, u32]
    L.x3_graph_begin.argtypes = [vp]
    L.x3_graph_end.argtypes = [vp, C.POINTER(vp)]
    L.x3_graph_launch.argtypes = [vp, vp]
    L.x3_graph_destroy.argtypes = [vp]
    L.x3_graph_destroy.restype = None
    L.x3_seg_index_entries.argtypes = [u64, PP, u32]
    L.x3_seg_index_entries.restype = u64
    L.x3_seg_index_build_dev.argtypes = [vp, vp, u64, vp, u64, PP, vp, u32]
    L.x3_decode_dev_seg.argtypes = [vp, vp, u64, vp, u64, C.POINTER(Batch), vp, PP, vp, u64, vp, vp, u32, i32]
    L.x3_index_dev.argtypes = [vp, vp, u64, u64, vp, vp, C.POINTER(u64), C.POINTER(u64), C.POINTER(i32)]
    L.x3_decode_stream_dev.argtypes = [vp, vp, u64, PP, vp, u64, C.POINTER(u64), C.POINTER(u64), C.POINTER(u64)]
    L.x3_sample_offsets_dev.argtypes = [vp, vp, u64, vp, u64, vp]
    L.x3_decode_windows_dev.argtypes = [vp, vp, u64, vp, vp, u64, PP, vp, u32, vp, u64, u32, vp, i32, vp]
    L.x3_decode_windows_result.argtypes = [vp, C.POINTER(u64), C.POINTER(u64), C.POINTER(i32)]
    L.x3_decode_ranges_dev.argtypes = [vp, vp, u64, vp, vp, u64, PP, vp, u32, vp, vp, u64, u64, vp, u64, i32, vp, vp]
    L.x3_corpus_ranges_dev.argtypes = [vp, vp, vp, vp, vp, u64, u64, vp, u64, i32, vp, vp]
    L.x3_decode_ranges_result.argtypes = [vp, C.POINTER(u64), C.POINTER(u64), C.POINTER(i32), C.POINTER(u64)]
    L.x3_decode_streams_dev.argtypes = [vp, vp, u64, vp, vp, u64, u32, PP, vp, u64, i32, vp]
    L.x3_decode_streams_result.argtypes = [vp, C.POINTER(u64), C.POINTER(u64), C.POINTER(i32)]
    L.x3_corpus_build.argtypes = [vp, vp, u64, vp, vp, u64, u32, PP, u32, C.POINTER(vp)]
    L.x3_corpus_info.argtypes = [vp, C.POINTER(u64), C.POINTER(u64), C.POINTER(u64), C.POINTER(u32)]
    L.x3_corpus_entries.argtypes = [vp, vp]
    L.x3_corpus_seg_index.argtypes = [vp, C.POINTER(vp), C.POINTER(u64)]
    L.x3_corpus_entries_dev.argtypes = [vp, C.POINTER(vp)]
    L.x3_corpus_windows_dev.argtypes = [vp, vp, vp, vp, u64, u32, vp, i32, vp]
    L.x3_corpus_destroy.argtypes = [vp]
    L.x3_levels_dev.argtypes = [vp, vp, u64, vp, vp, u64, PP, vp, u32, u64, vp, u64, vp]
    L.x3_levels_result.argtypes = [vp, C.POINTER(u64), C.POINTER(u64), C.POINTER(i32)]
    L.x3_corpus_levels_rows.argtypes = [vp, u64, vp]
    L.x3_corpus_levels_dev.argtypes = [vp, vp, u64, vp, u64, vp]
    L.x3_signal_levels_dev.argtypes = [vp, vp, u64, vp, vp, u64, PP, vp, u32, u64, vp, u64, vp, C.c_int]
    L.x3_corpus_signal_levels_dev.argtypes = [vp, vp, u64, vp, u64, vp, C.c_int]
    L.x3_fir_levels_dev.argtypes = [vp, vp, u64, vp, vp, u64, PP, vp, u32, u64, vp, u64, vp, C.POINTER(LevelFir)]
    L.x3_corpus_fir_levels_dev.argtypes = [vp, vp, u64, vp, u64, vp, C.POINTER(LevelFir)]
    L.x3_tone_levels_dev.argtypes = [vp, vp, u64, vp, vp, u64, PP, vp, u32, u64, vp, u64, vp, C.POINTER(LevelTone)]
    L.x3_corpus_tone_levels_dev.argtypes = [vp, vp, u64, vp, u64, vp, C.POINTER(LevelTone)]
    L.x3_tone_power_levels_dev.argtypes = [vp, vp, u64, vp]
    L.x3_tone_bank_levels_dev.argtypes = [vp, vp, u64, vp, vp, u64, PP, vp, u32, u64, vp, u64, vp, C.POINTER(LevelToneBank)]
    L.x3_corpus_tone_bank_levels_dev.argtypes = [vp, vp, u64, vp, u64, vp, C.POINTER(LevelToneBank)]
    L.x3_events_dev.argtypes = [vp, vp, u64, u64, vp, C.POINTER(EventRule), vp, vp, vp, u64, vp]
    L.x3_corpus_events_dev.argtypes = [vp, vp, vp, u64, u64, C.POINTER(EventRule), vp, vp, vp, vp, u64, vp]
    L.x3_events_result.argtypes = [vp, C.POINTER(u64)]
    L.x3_level_quantiles_dev.argtypes = [vp, vp, u64, u64, vp, C.c_int, C.POINTER(C.c_uint32), C.c_uint32, vp, vp]
    L.x3_corpus_level_quantiles_dev.argtypes = [vp, vp, vp, u64, u64, C.c_int, C.POINTER(C.c_uint32), C.c_uint32, vp, vp]
    L.x3_level_quantiles_result.argtypes = [vp, C.POINTER(u64), C.POINTER(u64)]
    L.x3_level_thresholds_dev.argtypes = [vp, vp, u64, u64, vp, C.POINTER(ThresholdRule), vp]
    L.x3_corpus_level_thresholds_dev.argtypes = [vp, vp, vp, u64, u64, C.POINTER(ThresholdRule), vp]
    L.x3_events_adaptive_dev.argtypes = [vp, vp, u64, u64, vp, C.POINTER(EventRule), vp, vp, vp, vp, u64, vp]
    L.x3_corpus_events_adaptive_dev.argtypes = [vp, vp, vp, u64, u64, C.POINTER(EventRule), vp, vp, vp, vp, vp, u64, vp]
    L.x3_plane_events_dev.argtypes = [vp, vp, u64, u64, u64, vp, C.POINTER(PlaneEventRule), vp, vp, vp, vp, vp, u64, vp]
    L.x3_corpus_plane_events_dev.argtypes = [vp, vp, vp, u64, u64, u64, C.POINTER(PlaneEventRule), vp, vp, vp, vp, vp, vp, u64, vp]
    L.x3_range_levels_dev.argtypes = [vp, vp, u64, vp, vp, u64, PP, vp, u32, vp, vp, u64, u64, u64, vp, u64, vp, vp]
    L.x3_corpus_range_levels_dev.argtypes = [vp, vp, vp, vp, vp, u64, u64, u64, vp, u64, vp, vp]
    L.x3_signal_range_levels_dev.argtypes = [vp, vp, u64, vp, vp, u64, PP, vp, u32, vp, vp, u64, u64, u64, vp, u64, vp, vp, C.c_int]
    L.x3_corpus_signal_range_levels_dev.argtypes = [vp, vp, vp, vp, vp, u64, u64, u64, vp, u64, vp, vp, C.c_int]
    L.x3_fir_range_levels_dev.argtypes = [vp, vp, u64, vp, vp, u64, PP, vp, u32, vp, vp, u64, u64, u64, vp, u64, vp, vp,
                                          C.POINTER(LevelFir)]
    L.x3_corpus_fir_range_levels_dev.argtypes = [vp, vp, vp, vp, vp, u64, u64, u64, vp, u64, vp, vp, C.POINTER(LevelFir)]
    L.x3_tone_range_levels_dev.argtypes = [vp, vp, u64, vp, vp, u64, PP, vp, u32, vp, vp, u64, u64, u64, vp, u64, vp, vp,
                                           C.POINTER(LevelTone)]
    L.x3_corpus_tone_range_levels_dev.argtypes = [vp, vp, vp, vp, vp, u64, u64, u64, vp, u64, vp, vp, C.POINTER(LevelTone)]
    L.x3_tone_bank_range_levels_dev.argtypes = [vp, vp, u64, vp, vp, u64, PP, vp, u32, vp, vp, u64, u64, u64, vp, u64, vp, vp,
                                                C.POINTER(LevelToneBank)]
    L.x3_corpus_tone_bank_range_levels_dev.argtypes = [vp, vp, vp, vp, vp, u64, u64, u64, vp, u64, vp, vp,
                                                       C.POINTER(LevelToneBank)]
    L.x3_range_levels_result.argtypes = [vp, C.POINTER(u64), C.POINTER(u64), C.POINTER(i32), C.POINTER(u64)]
    L.x3_spectra_rows_dev.argtypes = [vp, vp, u64, vp, vp, vp, u64, C.POINTER(SpectraRule), u64, vp, u64, vp, vp]
    L.x3_spectra_levels_dev.argtypes = [vp, vp, u64, vp, vp, vp, u64, C.POINTER(SpectraRule), C.POINTER(SpectraFold), u64, vp, u64,
                                        vp, vp]
    L.x3_spectra_result.argtypes = [vp, C.POINTER(u64), C.POINTER(u64), C.POINTER(i32), C.POINTER(u64)]
    L.x3_corpus_destroy.restype = None
    L.x3_synth.argtypes = [i32, u64, u64, u64, vp]
    L.x3_synth_dev.argtypes = [vp, i32, u64, u64, u64, vp]
    L.x3_dev_alloc.argtypes = [vp, u64, C.POINTER(vp)]
    L.x3_dev_free.argtypes = [vp, vp]
    L.x3_dev_upload.argtypes = [vp, vp, vp, u64]
    L.x3_dev_download.argtypes = [vp, vp, vp, u64]
    L.x3_bitreader_new.argtypes = [vp, vp, u64, C.POINTER(vp)]
    L.x3_bitreader_read_nbits.argtypes = [vp, u32, C.POINTER(u32)]
    L.x3_bitreader_count_zero_bits.argtypes = [vp, C.POINTER(u32)]
    L.x3_bitreader_inc_bits.argtypes = [vp, u32]
    L.x3_bitreader_state.argtypes = [vp, C.POINTER(u64), C.POINTER(u32), C.POINTER(u32)]
    L.x3_bitreader_free.restype = None
    L.x3_bitreader_free.argtypes = [vp]
    L.x3_decode_block.argtypes = [vp, vp, u32, C.POINTER(C.c_int16), PP]
    L.x3_bitpacker_new.argtypes = [vp, vp, u64, u64, C.POINTER(vp)]
    L.x3_bitpacker_write_bits.argtypes = [vp, u64, u32]
    L.x3_bitpacker_write_packed_zeros.argtypes = [vp, u32]
    L.x3_bitpacker_write_bytes.argtypes = [vp, vp, u64]
    L.x3_bitpacker_inc_counter_n_bytes.argtypes = [vp, u64]
    L.x3_bitpacker_word_align.argtypes = [vp]
    L.x3_bitpacker_finish.argtypes = [vp, C.POINTER(u64), C.POINTER(C.c_uint16), C.POINTER(u64)]
    L.x3_bitpacker_peek.argtypes = [vp, C.POINTER(u64), C.POINTER(C.c_uint16)]
    L.x3_bitpacker_take.argtypes = [vp, vp, u64, C.POINTER(u64), C.POINTER(u64), C.POINTER(C.c_uint16)]
    L.x3_bitpacker_free.restype = None
    L.x3_bitpacker_free.argtypes = [vp]
    L.x3_reader_open.argtypes = [vp, C.c_char_p, C.POINTER(vp)]
    L.x3_reader_open_mem.argtypes = [vp, vp, u64, C.POINTER(vp)]
    L.x3_reader_spec.argtypes = [vp, C.POINTER(u32), PP, C.POINTER(C.c_uint8)]
    L.x3_reader_next_frame.argtypes = [vp, vp, u64, C.POINTER(u64)]
    L.x3_reader_frame_errors.restype = u64
    L.x3_reader_frame_errors.argtypes = [vp]
    L.x3_reader_position.restype = u64
    L.x3_reader_position.argtypes = [vp]
    L.x3_reader_close.restype = None
    L.x3_reader_close.argtypes = [vp]
    L.x3_shard_unique_id.argtypes = [vp]
    L.x3_shard_create.argtypes = [vp, vp, i32, i32, C.POINTER(vp)]
    L.x3_shard_destroy.restype = None
    L.x3_shard_destroy.argtypes = [vp]
    L.x3_shard_rank.argtypes = [vp]
    L.x3_shard_world.argtypes = [vp]
    L.x3_shard_frame_range.restype = None
    L.x3_shard_frame_range.argtypes = [u64, i32, i32, C.POINTER(u64), C.POINTER(u64)]
    L.x3_shard_sample_range.restype = None
    L.x3_shard_sample_range.argtypes = [u64, PP, i32, i32, C.POINTER(u64), C.POINTER(u64)]
    L.x3_shard_offsets.restype = None
    L.x3_shard_offsets.argtypes = [C.POINTER(u64), i32, C.POINTER(u64)]
    L.x3_shard_exchange_lengths.argtypes = [vp, vp, vp]
    L.x3_shard_exchange_length_value.argtypes = [vp, u64, vp]
    L.x3_shard_lengths.argtypes = [vp, C.POINTER(u64)]
    L.x3_shard_gather.argtypes = [vp, vp, C.POINTER(u64), i32, vp, u64, C.POINTER(u64)]
    L.x3_shard_gather_async.argtypes = [vp, vp, C.POINTER(u64), i32, vp, u64, C.POINTER(u64)]
    L.x3_shard_gather_wait.argtypes = [vp, i32]
    L.x3_shard_write_at.argtypes = [vp, vp, C.POINTER(u64), i32, u64, C.POINTER(u64)]
    L.x3_mgpu_create.argtypes = [C.POINTER(i32), i32, C.POINTER(vp)]
    L.x3_mgpu_destroy.restype = None
    L.x3_mgpu_destroy.argtypes = [vp]
    L.x3_mgpu_devices.argtypes = [vp]
    L.x3_mgpu_ctx.restype = vp
    L.x3_mgpu_ctx.argtypes = [vp, i32]
    L.x3_mgpu_shard.restype = vp
    L.x3_mgpu_shard.argtypes = [vp, i32]
    L.x3_mgpu_last_error.restype = C.c_char_p
    L.x3_mgpu_last_error.argtypes = [vp]
    L.x3_mgpu_encode.argtypes = [vp, vp, u64, u32, PP, vp, u64, u64, C.POINTER(u64), vp]
    L.x3_mgpu_decode_stream.argtypes = [vp, vp, u64, PP, vp, u64, C.POINTER(u64), C.POINTER(u64), C.POINTER(u64)]
    L.x3_tune_candidate.argtypes = [u32, u32, PP]
    L.x3_tuner_create.argtypes = [vp, u32, C.POINTER(vp)]
    L.x3_tuner_add_dev.argtypes = [vp, vp, C.POINTER(Batch)]
    L.x3_tuner_result.argtypes = [vp, PP, C.POINTER(u64), vp]
    L.x3_tuner_max_payloads.argtypes = [vp, vp]
    L.x3_tuner_reset.argtypes = [vp]
    L.x3_tuner_destroy.restype = None
    L.x3_tuner_destroy.argtypes = [vp]
    L.x3_tune.argtypes = [vp, vp, u64, u32, PP, C.POINTER(u64), vp]
    L.x3_x3a_encode_tuned.argtypes = [vp, vp, u64, u32, vp, u64, C.POINTER(u64), vp, PP]
    _lib = L
    return L


# ---- sharding arithmetic (host only: works without a GPU)

def shard_frame_range(n_frames, rank, world):
    a, c = C.c_uint64(0), C.c_uint64(0)
    lib().x3_shard_frame_range(n_frames, rank, world, C.byref(a), C.byref(c))
    return a.value, c.value


def shard_sample_range(n_samples, params, rank, world):
    a, c = C.c_uint64(0), C.c_uint64(0)
    lib().x3_shard_sample_range(n_samples, C.byref(params), rank, world, C.byref(a), C.byref(c))
    return a.value, c.value


def shard_offsets(lengths):
    n = len(lengths)
    src = (C.c_uint64 * n)(*[int(v) for v in lengths])
    dst = (C.c_uint64 * (n + 1))()
    lib().x3_shard_offsets(src, n, dst)
    return list(dst)


def shard_unique_id():
    """ncclGetUniqueId through the library: 128 bytes, made by rank 0 and handed to the other ranks out of band"""
    buf = (C.c_uint8 * 128)()
    rc = lib().x3_shard_unique_id(buf)
    if rc:
        raise X3Error(rc, "x3_shard_unique_id (librccl not available?)")
    return bytes(buf)


class Reader:
    """X3aReader (decodefile.rs:47-137) over a file path or over archive bytes: spec() and next_frame()"""

    def __init__(self, ctx, source):
        self._h = C.c_void_p()
        self.ctx = ctx
        if isinstance(source, (str, bytes, os.PathLike)) and not isinstance(source, bytes):
            rc = lib().x3_reader_open(ctx._h, os.fsencode(source), C.byref(self._h))
        else:
            self._keep = np.ascontiguousarray(source, dtype=np.uint8)   # borrowed by the reader
            rc = lib().x3_reader_open_mem(ctx._h, self._keep.ctypes.data, self._keep.size, C.byref(self._h))
        self.rc = rc
        self._buf = np.zeros(65536, dtype=np.int16)

    def spec(self):
        rate, p, ch = C.c_uint32(0), Params(), C.c_uint8(0)
        lib().x3_reader_spec(self._h, C.byref(rate), C.byref(p), C.byref(ch))
        return rate.value, p, ch.value

    def next_frame(self):
        """-> (rc, samples or None): None = Ok(None) of the reference"""
        n = C.c_uint64(0)
        rc = lib().x3_reader_next_frame(self._h, self._buf.ctypes.data, self._buf.size, C.byref(n))
        return rc, (self._buf[: n.value].copy() if (rc == 0 and n.value) else None)

    def frame_errors(self):
        return lib().x3_reader_frame_errors(self._h)

    def position(self):
        return lib().x3_reader_position(self._h)

    def close(self):
        if self._h:
            lib().x3_reader_close(self._h)
            self._h = C.c_void_p()


class Shard:
    """one rank of a group of GPUs (x3_shard): RCCL communicator on the context's device and stream"""

    def __init__(self, ctx, unique_id, rank, world):
        self._h = C.c_void_p()
        self.ctx, self.rank, self.world = ctx, rank, world
        buf = (C.c_uint8 * 128).from_buffer_copy(unique_id)
        rc = lib().x3_shard_create(ctx._h, buf, rank, world, C.byref(self._h))
        if rc:
            raise X3Error(rc, "x3_shard_create: " + ctx.last_error())

    def close(self):
        if self._h:
            lib().x3_shard_destroy(self._h)
            self._h = C.c_void_p()

    def exchange_lengths(self, d_len, d_lengths=None):
        rc = lib().x3_shard_exchange_lengths(self._h, d_len, d_lengths)
        if rc:
            raise X3Error(rc, "x3_shard_exchange_lengths: " + self.ctx.last_error())

    def lengths(self):
        out = (C.c_uint64 * self.world)()
        rc = lib().x3_shard_lengths(self._h, out)
        if rc:
            raise X3Error(rc, "x3_shard_lengths: " + self.ctx.last_error())
        return list(out)

    def gather(self, d_sub, lengths, root, d_dst, dst_cap, overlapped=False):
        """reassembly on `root`; overlapped=True: on the shard's own stream and communicator, beside whatever the context
        does next (x3_shard_gather_async) -- d_sub / d_dst stay untouched until gather_wait()"""
        src = (C.c_uint64 * self.world)(*[int(v) for v in lengths])
        tot = C.c_uint64(0)
        fn = lib().x3_shard_gather_async if overlapped else lib().x3_shard_gather
        rc = fn(self._h, d_sub, src, root, d_dst, dst_cap, C.byref(tot))
        if rc:
            raise X3Error(rc, "x3_shard_gather: " + self.ctx.last_error())
        return tot.value

    def write_at(self, d_sub, lengths, fd, base=0):
        """sharded reassembly (x3_shard_write_at): this rank's sub-stream to byte base + starts[rank] of the file `fd`"""
        src = (C.c_uint64 * self.world)(*[int(v) for v in lengths])
        tot = C.c_uint64(0)
        rc = lib().x3_shard_write_at(self._h, d_sub, src, fd, base, C.byref(tot))
        if rc:
            raise X3Error(rc, "x3_shard_write_at: " + self.ctx.last_error())
        return tot.value

    def gather_wait(self, on_stream=True):
        rc = lib().x3_shard_gather_wait(self._h, 1 if on_stream else 0)
        if rc:
            raise X3Error(rc, "x3_shard_gather_wait: " + self.ctx.last_error())


class MultiGpu:
    """all GPUs from one process (x3_mgpu): host buffers in and out, same bytes as Context.encode / decode_stream"""

    def __init__(self, devices):
        self._h = C.c_void_p()
        arr = (C.c_int * len(devices))(*devices)
        rc = lib().x3_mgpu_create(arr, len(devices), C.byref(self._h))
        if rc:
            raise X3Error(rc, "x3_mgpu_create")

    def close(self):
        if self._h:
            lib().x3_mgpu_destroy(self._h)
            self._h = C.c_void_p()

    def last_error(self):
        return lib().x3_mgpu_last_error(self._h).decode()

    def encode(self, wav, params=None, start_pos=0, cap=None, n_channels=1):
        params = params or Params.default()
        wav = np.ascontiguousarray(wav, dtype=np.int16)
        if cap is None:
            cap = start_pos + lib().x3_encode_bound(wav.size, C.byref(params)) + 1
        out = np.zeros(max(cap, 1), dtype=np.uint8)
        pos = C.c_uint64(0)
        stats = np.zeros(6, dtype=np.uint64)
        rc = lib().x3_mgpu_encode(self._h, wav.ctypes.data, wav.size, n_channels, C.byref(params), out.ctypes.data,
                                  cap, start_pos, C.byref(pos), stats.ctypes.data)
        return rc, out[: min(pos.value, cap)].copy(), stats

    def decode_stream(self, x3, params=None, wav_cap=None):
        params = params or Params.default()
        x3 = np.ascontiguousarray(x3, dtype=np.uint8)
        if wav_cap is None:
            wav_cap = max(1, x3.size * 16)
        wav = np.zeros(wav_cap, dtype=np.int16)
        n, fok, ferr = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        rc = lib().x3_mgpu_decode_stream(self._h, x3.ctypes.data, x3.size, C.byref(params), wav.ctypes.data, wav_cap,
                                         C.byref(n), C.byref(fok), C.byref(ferr))
        return rc, wav[: n.value].copy(), fok.value, ferr.value


def place_buffers(ctx, params, d_wav, n, d_streams, cap, d_frame_offsets, d_backs, warm=4, steps=8):
    """x3_place_buffers (include/x3hip.h, "Placement"): where in HBM the stream and the decoded samples lie decides the decode
    phase's pace by up to 10 % -- per PAIR of buffers, reproducibly within a process, and not by anything an address shows
    (profiles/r6/decoder_modes.txt).  Times `steps` round trips (after `warm` untimed ones) on every (stream buffer, sample
    buffer) pair and returns ms_per_step[i][j]; the caller keeps the best pair and frees the rest."""
    ns, nb = len(d_streams), len(d_backs)
    streams = (C.c_void_p * ns)(*d_streams)
    backs = (C.c_void_p * nb)(*d_backs)
    ms = (C.c_double * (ns * nb))()
    L = lib()
    L.x3_place_buffers.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(Params), C.c_void_p, C.c_uint32, C.c_uint64,
                                   C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p]
    L.x3_place_buffers.restype = C.c_int
    rc = L.x3_place_buffers(ctx._h, d_wav, n, C.byref(params), streams, ns, cap, d_frame_offsets, backs, nb, warm, steps, ms)
    if rc:
        raise X3Error(rc, "x3_place_buffers: " + ctx.last_error())
    return [[ms[i * nb + j] for j in range(nb)] for i in range(ns)]


def strerror(rc):
    return lib().x3_strerror(rc).decode()


class X3Error(RuntimeError):
    def __init__(self, rc, what=""):
        self.rc = rc
        super().__init__("%s: %s (%d)" % (what, strerror(rc), rc))


def tune_candidate(index, spf=TUNE_DEFAULT_SPF):
    """candidate `index` of the tuning grid at frame length spf -> (rc, Params)"""
    p = Params()
    rc = lib().x3_tune_candidate(index, spf, C.byref(p))
    return rc, p


class Tuner:
    """x3_tuner: per-candidate encoded sizes accumulated over device-resident batches (include/x3hip.h)"""

    def __init__(self, ctx, spf=TUNE_DEFAULT_SPF):
        self._ctx = ctx
        self._h = C.c_void_p()
        rc = lib().x3_tuner_create(ctx._h, spf, C.byref(self._h))
        if rc:
            raise X3Error(rc, "x3_tuner_create")
        self.spf = spf

    def add_dev(self, d_wav, n_per_clip, clip_stride=None, n_clips=1):
        """enqueue one batch (x3_encode_dev's layout) -> status"""
        b = Batch(n_per_clip, n_per_clip if clip_stride is None else clip_stride, n_clips)
        return lib().x3_tuner_add_dev(self._h, C.c_void_p(d_wav), C.byref(b))

    def result(self):
        """-> (rc, best Params, best_bytes, sizes[2184] uint64)"""
        p = Params()
        bb = C.c_uint64(0)
        sizes = np.zeros(TUNE_CANDIDATES, dtype=np.uint64)
        rc = lib().x3_tuner_result(self._h, C.byref(p), C.byref(bb), sizes.ctypes.data)
        return rc, p, bb.value, sizes

    def max_payloads(self):
        out = np.zeros(TUNE_CANDIDATES, dtype=np.uint32)
        rc = lib().x3_tuner_max_payloads(self._h, out.ctypes.data)
        if rc:
            raise X3Error(rc, "x3_tuner_max_payloads")
        return out

    def reset(self):
        return lib().x3_tuner_reset(self._h)

    def close(self):
        if self._h:
            lib().x3_tuner_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


SYNTH_ZEROS, SYNTH_WHITE, SYNTH_HYDROPHONE, SYNTH_SINE, SYNTH_WALK = range(5)


def synth(kind, seed, start, n):
    """host-side synthetic samples (bit-identical to Context.synth_dev)"""
    out = np.empty(n, dtype=np.int16)
    rc = lib().x3_synth(kind, seed, start, n, out.ctypes.data)
    if rc:
        raise X3Error(rc, "x3_synth")
    return out


def write_frame_header(num_samples, ident, payload_len, payload_crc):
    out = np.zeros(20, dtype=np.uint8)
    lib().x3_write_frame_header(num_samples, ident, payload_len, payload_crc, out.ctypes.data)
    return out


def archive_header_write(sample_rate, params=None, cap=1024):
    """-> (rc, header bytes)"""
    params = params or Params.default()
    out = np.zeros(cap, dtype=np.uint8)
    n = C.c_uint64(0)
    rc = lib().x3_archive_header_write(sample_rate, C.byref(params), out.ctypes.data, cap, C.byref(n))
    return rc, out[: min(n.value, cap)].copy()


def archive_header_read(data):
    """-> (rc, sample_rate, Params, channels, header_size)"""
    b = np.ascontiguousarray(data, dtype=np.uint8)
    rate, p, ch, hs = C.c_uint32(0), Params(), C.c_uint8(0), C.c_uint64(0)
    rc = lib().x3_archive_header_read(b.ctypes.data, b.size, C.byref(rate), C.byref(p), C.byref(ch), C.byref(hs))
    return rc, rate.value, p, ch.value, hs.value


def read_frame_header(data):
    b = np.ascontiguousarray(data, dtype=np.uint8)
    h = FrameHeader()
    rc = lib().x3_read_frame_header(b.ctypes.data, b.size, C.byref(h))
    return rc, h


class Context:
    """One x3_ctx: a GPU + stream + scratch.  Not thread-safe."""

    def __init__(self, device=0, stream=None):
        self._h = C.c_void_p()
        L = lib()
        if stream is None:
            rc = L.x3_ctx_create(device, C.byref(self._h))
        else:
            rc = L.x3_ctx_create_on_stream(device, C.c_void_p(stream), C.byref(self._h))
        if rc:
            raise X3Error(rc, "x3_ctx_create (no usable HIP device? there is no CPU fallback)")

    def close(self):
        if self._h:
            if getattr(self, "_tone_table", None):
                self.free(self._tone_table)
                self._tone_table = None
            lib().x3_ctx_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def last_error(self):
        return lib().x3_last_error(self._h).decode()

    def set_option(self, name, value):
        """tuning / testing knobs (include/x3hip.h: x3_ctx_set_option)"""
        rc = lib().x3_ctx_set_option(self._h, name.encode(), int(value))
        if rc:
            raise X3Error(rc, "x3_ctx_set_option(%s)" % name)

    def get_option(self, name):
        v = C.c_longlong(0)
        rc = lib().x3_ctx_get_option(self._h, name.encode(), C.byref(v))
        if rc:
            raise X3Error(rc, "x3_ctx_get_option(%s)" % name)
        return v.value

    def sync(self):
        rc = lib().x3_ctx_sync(self._h)
        if rc:
            raise X3Error(rc, "x3_ctx_sync: " + self.last_error())

    # ---- host-buffer API (returns status codes, like the C ABI) ---------------------------
    def encode(self, wav, params=None, start_pos=0, cap=None, n_channels=1):
        """encoder::encode into a slice writer -> (rc, np.uint8 bytes[0:out_pos], stats[6])"""
        params = params or Params.default()
        wav = np.ascontiguousarray(wav, dtype=np.int16)
        if cap is None:
            cap = start_pos + lib().x3_encode_bound(wav.size, C.byref(params)) + 1
        out = np.zeros(max(cap, 1), dtype=np.uint8)
        pos = C.c_uint64(0)
        stats = np.zeros(6, dtype=np.uint64)
        rc = lib().x3_encode(self._h, wav.ctypes.data, wav.size, n_channels, C.byref(params), out.ctypes.data, cap,
                             start_pos, C.byref(pos), stats.ctypes.data)
        self.out_pos = pos.value
        return rc, out[: min(pos.value, cap)].copy(), stats

    def encode_frame(self, wav, params=None, start_pos=0, cap=None):
        params = params or Params.default()
        wav = np.ascontiguousarray(wav, dtype=np.int16)
        if cap is None:
            cap = start_pos + 64 + 3 * wav.size
        out = np.zeros(max(cap, 1), dtype=np.uint8)
        pos = C.c_uint64(0)
        stats = np.zeros(6, dtype=np.uint64)
        rc = lib().x3_encode_frame(self._h, wav.ctypes.data, wav.size, C.byref(params), out.ctypes.data, cap,
                                   start_pos, C.byref(pos), stats.ctypes.data)
        return rc, out[: min(pos.value, cap)].copy(), stats

    def encode_batch(self, clips, params=None, cap=None):
        params = params or Params.default()
        clips = [np.ascontiguousarray(c, dtype=np.int16) for c in clips]
        ptrs = (C.c_void_p * len(clips))(*[c.ctypes.data for c in clips])
        ns = (C.c_uint64 * len(clips))(*[c.size for c in clips])
        if cap is None:
            cap = sum(lib().x3_encode_bound(c.size, C.byref(params)) + 2 for c in clips)
        out = np.zeros(max(cap, 1), dtype=np.uint8)
        offs = (C.c_uint64 * (len(clips) + 1))()
        stats = np.zeros(6, dtype=np.uint64)
        rc = lib().x3_encode_batch(self._h, ptrs, ns, len(clips), C.byref(params), out.ctypes.data, cap, offs,
                                   stats.ctypes.data)
        return rc, out, list(offs), stats

    def decode_stream(self, x3, params=None, wav_cap=None):
        """-> (rc, samples, frames_ok, frame_errors)"""
        params = params or Params.default()
        x3 = np.ascontiguousarray(x3, dtype=np.uint8)
        if wav_cap is None:
            wav_cap = max(1, x3.size * 16)
        wav = np.zeros(wav_cap, dtype=np.int16)
        n, fok, ferr = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        rc = lib().x3_decode_stream(self._h, x3.ctypes.data, x3.size, C.byref(params), wav.ctypes.data, wav_cap,
                                    C.byref(n), C.byref(fok), C.byref(ferr))
        return rc, wav[: n.value].copy(), fok.value, ferr.value

    def encode_mc(self, wavs, params=None, start_pos=0, cap=None):
        """multi-channel extension (x3_encode_mc): wavs = equally long int16 arrays -> (rc, bytes, stats[6])"""
        params = params or Params.default()
        wavs = [np.ascontiguousarray(w, dtype=np.int16) for w in wavs]
        n = wavs[0].size
        assert all(w.size == n for w in wavs)
        L = lib()
        cap = len(wavs) * L.x3_encode_bound(n, C.byref(params)) + start_pos + 64 if cap is None else cap
        out = np.zeros(max(cap, 1), dtype=np.uint8)
        pos = C.c_uint64(0)
        stats = np.zeros(6, dtype=np.uint64)
        ptrs = (C.c_void_p * len(wavs))(*[w.ctypes.data for w in wavs])
        L.x3_encode_mc.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64,
                                   C.c_uint64, C.c_void_p, C.c_void_p]
        rc = L.x3_encode_mc(self._h, ptrs, len(wavs), n, C.byref(params), out.ctypes.data, cap, start_pos, C.byref(pos),
                            stats.ctypes.data)
        return rc, out[: pos.value].copy(), stats

    def decode_stream_mc(self, x3, n_ch, params=None, wav_cap=None):
        """-> (rc, [samples of channel k], frames_ok, frame_errors)"""
        params = params or Params.default()
        x3 = np.ascontiguousarray(x3, dtype=np.uint8)
        if wav_cap is None:
            wav_cap = max(1, x3.size * 16)
        wavs = [np.zeros(wav_cap, dtype=np.int16) for _ in range(n_ch)]
        ptrs = (C.c_void_p * n_ch)(*[w.ctypes.data for w in wavs])
        n, fok, ferr = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        L = lib()
        L.x3_decode_stream_mc.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p,
                                          C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]
        rc = L.x3_decode_stream_mc(self._h, x3.ctypes.data, x3.size, n_ch, C.byref(params), ptrs, wav_cap, C.byref(n),
                                   C.byref(fok), C.byref(ferr))
        return rc, [w[: n.value].copy() for w in wavs], fok.value, ferr.value

    def decode_prefetch(self, x3=None, params=None):
        """announce a frame stream (a contiguous uint8 array, kept alive here) for decode_frame loops; None drops it"""
        if x3 is None:
            self._prefetched = None
            return lib().x3_decode_prefetch(self._h, None, 0, None)
        params = params or Params.default()
        assert x3.dtype == np.uint8 and x3.flags.c_contiguous
        self._prefetched = x3
        return lib().x3_decode_prefetch(self._h, x3.ctypes.data, x3.size, C.byref(params))

    def decode_frame(self, payload, samples, params=None, wav_cap=None):
        params = params or Params.default()
        payload = np.ascontiguousarray(payload, dtype=np.uint8)
        wav_cap = samples if wav_cap is None else wav_cap
        wav = np.zeros(max(wav_cap, 1), dtype=np.int16)
        n = C.c_uint64(0)
        rc = lib().x3_decode_frame(self._h, payload.ctypes.data, payload.size, wav.ctypes.data, wav_cap,
                                   C.byref(params), samples, C.byref(n))
        return rc, wav[: n.value].copy()

    def x3a_encode(self, wav, sample_rate, cap=None):
        """wav_to_x3a in memory -> (rc, .x3a bytes, stats)"""
        wav = np.ascontiguousarray(wav, dtype=np.int16)
        p = Params.default()
        if cap is None:
            cap = 1024 + lib().x3_encode_bound(wav.size, C.byref(p))
        out = np.zeros(max(cap, 1), dtype=np.uint8)
        n = C.c_uint64(0)
        stats = np.zeros(6, dtype=np.uint64)
        rc = lib().x3_x3a_encode(self._h, wav.ctypes.data, wav.size, sample_rate, out.ctypes.data, cap, C.byref(n),
                                 stats.ctypes.data)
        return rc, out[: min(n.value, cap)].copy(), stats

    def tune(self, wav, spf=TUNE_DEFAULT_SPF):
        """x3_tune on host samples -> (Params, best_bytes, sizes[2184] uint64); raises X3Error on failure"""
        wav = np.ascontiguousarray(wav, dtype=np.int16)
        p = Params()
        bb = C.c_uint64(0)
        sizes = np.zeros(TUNE_CANDIDATES, dtype=np.uint64)
        rc = lib().x3_tune(self._h, wav.ctypes.data if wav.size else None, wav.size, spf, C.byref(p), C.byref(bb),
                           sizes.ctypes.data)
        if rc:
            raise X3Error(rc, "x3_tune")
        return p, bb.value, sizes

    def x3a_encode_tuned(self, wav, sample_rate, cap=None):
        """x3a_encode with the parameters x3_tune chooses -> (rc, .x3a bytes, stats, chosen Params)"""
        wav = np.ascontiguousarray(wav, dtype=np.int16)
        if cap is None:
            cap = 1024 + lib().x3_encode_bound(wav.size, C.byref(Params.make(block_len=10, blocks_per_frame=1000)))
        out = np.zeros(max(cap, 1), dtype=np.uint8)
        n = C.c_uint64(0)
        stats = np.zeros(6, dtype=np.uint64)
        p = Params()
        rc = lib().x3_x3a_encode_tuned(self._h, wav.ctypes.data, wav.size, sample_rate, out.ctypes.data, cap, C.byref(n),
                                       stats.ctypes.data, C.byref(p))
        return rc, out[: min(n.value, cap)].copy(), stats, p

    def x3a_decode(self, x3a, wav_cap=None):
        """x3a_to_wav in memory -> (rc, samples, sample_rate, frames_ok, frame_errors)"""
        x3a = np.ascontiguousarray(x3a, dtype=np.uint8)
        if wav_cap is None:
            wav_cap = max(1, x3a.size * 16)
        wav = np.zeros(wav_cap, dtype=np.int16)
        n, rate, fok, ferr = C.c_uint64(0), C.c_uint32(0), C.c_uint64(0), C.c_uint64(0)
        rc = lib().x3_x3a_decode(self._h, x3a.ctypes.data, x3a.size, wav.ctypes.data, wav_cap, C.byref(n),
                                 C.byref(rate), C.byref(fok), C.byref(ferr))
        return rc, wav[: n.value].copy(), rate.value, fok.value, ferr.value


    def wav_to_x3a(self, wav_path, x3a_path):
        """encodefile::wav_to_x3a on files (streamed through the GPU) -> (rc, stats[6])"""
        stats = np.zeros(6, dtype=np.uint64)
        rc = lib().x3_wav_to_x3a(self._h, os.fsencode(wav_path), os.fsencode(x3a_path), stats.ctypes.data)
        return rc, stats

    def x3a_to_wav(self, x3a_path, wav_path):
        """decodefile::x3a_to_wav on files -> (rc, samples written, frame_errors)"""
        n, ferr = C.c_uint64(0), C.c_uint64(0)
        rc = lib().x3_x3a_to_wav(self._h, os.fsencode(x3a_path), os.fsencode(wav_path), C.byref(n), C.byref(ferr))
        return rc, n.value, ferr.value

    def crc16(self, data):
        b = np.ascontiguousarray(np.frombuffer(bytes(data), dtype=np.uint8)) if not isinstance(data, np.ndarray) \
            else np.ascontiguousarray(data, dtype=np.uint8)
        crc = C.c_uint16(0)
        rc = lib().x3_crc16(self._h, b.ctypes.data if b.size else None, b.size, C.byref(crc))
        if rc:
            raise X3Error(rc, "x3_crc16: " + self.last_error())
        return crc.value

    # ---- device-resident API (raw device pointers as ints, e.g. torch.Tensor.data_ptr()) -----
    def encode_dev(self, d_wav, n_per_clip, params, d_out, out_cap, start_pos=0, d_frame_offsets=None, n_clips=1,
                   clip_stride=None):
        b = Batch(n_per_clip, n_per_clip if clip_stride is None else clip_stride, n_clips)
        return lib().x3_encode_dev(self._h, d_wav, C.byref(b), C.byref(params), d_out, out_cap, start_pos,
                                   d_frame_offsets)

    def encode_dev_seg(self, d_wav, n_per_clip, params, d_out, out_cap, d_seg_index, seg_blocks, start_pos=0, d_frame_offsets=None,
                       n_clips=1, clip_stride=None):
        """x3_encode_dev_seg: encode and leave the segment index of the stream in d_seg_index"""
        b = Batch(n_per_clip, n_per_clip if clip_stride is None else clip_stride, n_clips)
        return lib().x3_encode_dev_seg(self._h, d_wav, C.byref(b), C.byref(params), d_out, out_cap, start_pos,
                                       d_frame_offsets, d_seg_index, seg_blocks)

    def encode_frames_dev(self, d_wav, src_offsets, src_samples, params, d_out, out_cap, start_pos=0, d_frame_offsets=None):
        """x3_encode_frames_dev: frame f = src_samples[f] samples at d_wav + src_offsets[f] (host arrays)"""
        so = np.ascontiguousarray(src_offsets, dtype=np.uint64)
        sn = np.ascontiguousarray(src_samples, dtype=np.uint32)
        assert so.size == sn.size
        return lib().x3_encode_frames_dev(self._h, d_wav, so.ctypes.data, sn.ctypes.data, so.size, C.byref(params), d_out,
                                          out_cap, start_pos, d_frame_offsets)

    def encode_result(self):
        pos = C.c_uint64(0)
        stats = np.zeros(6, dtype=np.uint64)
        rc = lib().x3_encode_result(self._h, C.byref(pos), stats.ctypes.data)
        return rc, pos.value, stats

    def decode_dev(self, d_x3, x3_len, d_frame_offsets, n_frames, params, d_wav, wav_cap, n_per_clip=None, n_clips=1,
                   clip_stride=None, d_wav_offsets=None, d_status=None):
        b = None
        if n_per_clip is not None:
            b = C.byref(Batch(n_per_clip, n_per_clip if clip_stride is None else clip_stride, n_clips))
        return lib().x3_decode_dev(self._h, d_x3, x3_len, d_frame_offsets, n_frames, b, d_wav_offsets,
                                   C.byref(params), d_wav, wav_cap, d_status)

    def decode_dev_seg(self, d_x3, x3_len, d_frame_offsets, n_frames, params, d_wav, wav_cap, d_seg_index, seg_blocks,
                       record=False, n_per_clip=None, n_clips=1, clip_stride=None, d_wav_offsets=None, d_status=None):
        """x3_decode_dev_seg: decode by the segment index (record=False) or decode frame by frame and record it"""
        b = None
        if n_per_clip is not None:
            b = C.byref(Batch(n_per_clip, n_per_clip if clip_stride is None else clip_stride, n_clips))
        return lib().x3_decode_dev_seg(self._h, d_x3, x3_len, d_frame_offsets, n_frames, b, d_wav_offsets,
                                       C.byref(params), d_wav, wav_cap, d_status, d_seg_index, seg_blocks, 1 if record else 0)

    def seg_index_build_dev(self, d_x3, x3_len, d_frame_offsets, n_frames, params, d_seg_index, seg_blocks):
        """x3_seg_index_build_dev: the segment index of any stream by a walk that stores no sample (asynchronous; every
        word of d_seg_index is written).  get_option("last_seg_index_irregular"): frames whose walk stopped early"""
        return lib().x3_seg_index_build_dev(self._h, d_x3, x3_len, d_frame_offsets, n_frames, C.byref(params), d_seg_index,
                                            seg_blocks)

    # ---- HIP graphs (x3_graph_*): record the device calls made between graph_begin() and graph_end(), replay them
    def graph_begin(self):
        rc = lib().x3_graph_begin(self._h)
        if rc:
            raise X3Error(rc, "x3_graph_begin: " + self.last_error())

    def graph_end(self):
        g = C.c_void_p()
        rc = lib().x3_graph_end(self._h, C.byref(g))
        if rc:
            raise X3Error(rc, "x3_graph_end: " + self.last_error())
        return g

    def graph_launch(self, g):
        rc = lib().x3_graph_launch(self._h, g)
        if rc:
            raise X3Error(rc, "x3_graph_launch: " + self.last_error())

    def graph_destroy(self, g):
        lib().x3_graph_destroy(g)

    def decode_result(self):
        fb, st, nb = C.c_uint64(0), C.c_int(0), C.c_uint64(0)
        rc = lib().x3_decode_result(self._h, C.byref(fb), C.byref(st), C.byref(nb))
        return rc, fb.value, st.value, nb.value

    def index_dev(self, d_x3, x3_len, max_frames, d_frame_offsets, d_wav_offsets):
        """GPU-side frame walk -> (rc, n_frames, n_samples, terminal)"""
        nf, ns, term = C.c_uint64(0), C.c_uint64(0), C.c_int(0)
        rc = lib().x3_index_dev(self._h, d_x3, x3_len, max_frames, d_frame_offsets, d_wav_offsets, C.byref(nf),
                                C.byref(ns), C.byref(term))
        return rc, nf.value, ns.value, term.value

    def decode_stream_dev(self, d_x3, x3_len, params, d_wav, wav_cap):
        """x3_decode_stream on device buffers -> (rc, n_samples, frames_ok, frame_errors)"""
        n, fok, ferr = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        rc = lib().x3_decode_stream_dev(self._h, d_x3, x3_len, C.byref(params), d_wav, wav_cap, C.byref(n),
                                        C.byref(fok), C.byref(ferr))
        return rc, n.value, fok.value, ferr.value

    def sample_offsets_dev(self, d_x3, x3_len, d_frame_offsets, n_frames, d_sample_offsets):
        """x3_sample_offsets_dev: d_sample_offsets[0..n_frames] = exclusive prefix of the headers' sample counts"""
        return lib().x3_sample_offsets_dev(self._h, d_x3, x3_len, d_frame_offsets, n_frames, d_sample_offsets)

    def decode_windows_dev(self, d_x3, x3_len, d_frame_offsets, d_sample_offsets, n_frames, params, d_starts, n_windows,
                           window_len, d_out, out_format, d_status, d_seg_index=None, seg_blocks=0):
        """x3_decode_windows_dev: n_windows rows of window_len samples (random access; asynchronous)"""
        return lib().x3_decode_windows_dev(self._h, d_x3, x3_len, d_frame_offsets, d_sample_offsets, n_frames,
                                           C.byref(params), d_seg_index, seg_blocks, d_starts, n_windows, window_len, d_out,
                                           out_format, d_status)

    def decode_windows_result(self):
        """-> (rc, n_bad, first_bad, first_bad_status) of the last decode_windows_dev"""
        nb, fb, st = C.c_uint64(0), C.c_uint64(0), C.c_int(0)
        rc = lib().x3_decode_windows_result(self._h, C.byref(nb), C.byref(fb), C.byref(st))
        return rc, nb.value, fb.value, st.value

    def decode_ranges_dev(self, d_x3, x3_len, d_frame_offsets, d_sample_offsets, n_frames, params, d_starts, d_lens, n_ranges,
                          row_stride, d_out, out_cap, out_format, d_out_offsets, d_status, d_seg_index=None, seg_blocks=0):
        """x3_decode_ranges_dev: range w = [d_starts[w], d_starts[w] + d_lens[w]), rows packed (row_stride 0) or padded;
        asynchronous"""
        return lib().x3_decode_ranges_dev(self._h, d_x3, x3_len, d_frame_offsets, d_sample_offsets, n_frames,
                                          C.byref(params), d_seg_index, seg_blocks, d_starts, d_lens, n_ranges, row_stride,
                                          d_out, out_cap, out_format, d_out_offsets, d_status)

    def decode_ranges_result(self):
        """-> (rc, n_bad, first_bad, first_bad_status, total_samples) of the last decode_ranges_dev / Corpus.ranges_into"""
        nb, fb, st, tot = C.c_uint64(0), C.c_uint64(0), C.c_int(0), C.c_uint64(0)
        rc = lib().x3_decode_ranges_result(self._h, C.byref(nb), C.byref(fb), C.byref(st), C.byref(tot))
        return rc, nb.value, fb.value, st.value, tot.value

    def levels_dev(self, d_x3, x3_len, d_frame_offsets, d_sample_offsets, n_frames, params, bin_len, d_levels, n_bins,
                   d_frame_status=None, d_seg_index=None, seg_blocks=0):
        """x3_levels_dev: n_bins x3_level records (LEVEL_DTYPE) of bins of bin_len positions (0: one bin); asynchronous"""
        return lib().x3_levels_dev(self._h, d_x3, x3_len, d_frame_offsets, d_sample_offsets, n_frames, C.byref(params),
                                   d_seg_index, seg_blocks, bin_len, d_levels, n_bins, d_frame_status)

    def signal_levels_dev(self, d_x3, x3_len, d_frame_offsets, d_sample_offsets, n_frames, params, bin_len, d_levels, n_bins,
                          d_frame_status=None, d_seg_index=None, seg_blocks=0, signal=LEVEL_SIGNAL_SAMPLES):
        """x3_signal_levels_dev: levels_dev of the samples (LEVEL_SIGNAL_SAMPLES) or of their first difference, clamped to 16
        bits (LEVEL_SIGNAL_DIFF); asynchronous, levels_result waits"""
        return lib().x3_signal_levels_dev(self._h, d_x3, x3_len, d_frame_offsets, d_sample_offsets, n_frames, C.byref(params),
                                          d_seg_index, seg_blocks, bin_len, d_levels, n_bins, d_frame_status, signal)

    def corpus_signal_levels_dev(self, corpus, bin_len, d_levels, n_rows, d_frame_status=None, signal=LEVEL_SIGNAL_SAMPLES):
        """x3_corpus_signal_levels_dev: corpus_levels_dev with a signal; asynchronous, levels_result waits"""
        return lib().x3_corpus_signal_levels_dev(self._h, corpus._h, bin_len, d_levels, n_rows, d_frame_status, signal)

    @staticmethod
    def _fir_arg(fir):
        """a Fir, a LevelFir or None (NULL, which the library refuses) as the calls' last argument"""
        if fir is None:
            return None
        return C.byref(fir.c_struct() if isinstance(fir, Fir) else fir)

    def fir_levels_dev(self, d_x3, x3_len, d_frame_offsets, d_sample_offsets, n_frames, params, bin_len, d_levels, n_bins,
                       d_frame_status=None, d_seg_index=None, seg_blocks=0, fir=None):
        """x3_fir_levels_dev: levels_dev of the samples behind an integer FIR filter (fir: a Fir, or a LevelFir as it is);
        asynchronous, levels_result waits"""
        return lib().x3_fir_levels_dev(self._h, d_x3, x3_len, d_frame_offsets, d_sample_offsets, n_frames, C.byref(params),
                                       d_seg_index, seg_blocks, bin_len, d_levels, n_bins, d_frame_status, self._fir_arg(fir))

    def corpus_fir_levels_dev(self, corpus, bin_len, d_levels, n_rows, d_frame_status=None, fir=None):
        """x3_corpus_fir_levels_dev: corpus_levels_dev behind an integer FIR filter; asynchronous, levels_result waits"""
        return lib().x3_corpus_fir_levels_dev(self._h, corpus._h, bin_len, d_levels, n_rows, d_frame_status, self._fir_arg(fir))

    def tone_table_dev(self):
        """-> the device pointer of the usual table (tone_table()), made at the first call and kept until close()"""
        if not getattr(self, "_tone_table", None):
            t = tone_table()
            p = self.alloc(t.nbytes)
            try:
                self.upload(p, t)
            except X3Error:
                self.free(p)
                raise
            self._tone_table = p
        return self._tone_table

    def _tone_arg(self, tone):
        """a Tone (with the context's usual table), a LevelTone as it is, or None (NULL, which the library refuses)"""
        if tone is None:
            return None
        return C.byref(LevelTone(tone.step, 0, self.tone_table_dev()) if isinstance(tone, Tone) else tone)

    def tone_levels_dev(self, d_x3, x3_len, d_frame_offsets, d_sample_offsets, n_frames, params, bin_len, d_levels, n_bins,
                        d_frame_status=None, d_seg_index=None, seg_blocks=0, tone=None):
        """x3_tone_levels_dev: n_bins x3_tone_level records (TONE_DTYPE), the quadrature sums of the bins' samples against
        one oscillator (tone: a Tone, or a LevelTone as it is); asynchronous, levels_result waits"""
        return lib().x3_tone_levels_dev(self._h, d_x3, x3_len, d_frame_offsets, d_sample_offsets, n_frames, C.byref(params),
                                        d_seg_index, seg_blocks, bin_len, d_levels, n_bins, d_frame_status, self._tone_arg(tone))

    def corpus_tone_levels_dev(self, corpus, bin_len, d_levels, n_rows, d_frame_status=None, tone=None):
        """x3_corpus_tone_levels_dev: corpus_levels_dev's rows as tone records, the phase restarting at every entry;
        asynchronous, levels_result waits"""
        return lib().x3_corpus_tone_levels_dev(self._h, corpus._h, bin_len, d_levels, n_rows, d_frame_status, self._tone_arg(tone))

    def _tone_bank_arg(self, tones):
        """a sequence of 1 .. TONE_BANK_MAX Tone (with the context's usual table), a LevelToneBank as it is, or None (NULL,
        which the library refuses)"""
        if tones is None:
            return None
        if isinstance(tones, LevelToneBank):
            return C.byref(tones)
        tones = tone_bank(tones)
        return C.byref(LevelToneBank(len(tones), 0, self.tone_table_dev(), (C.c_uint32 * TONE_BANK_MAX)(*[t.step for t in tones])))

    def tone_bank_levels_dev(self, d_x3, x3_len, d_frame_offsets, d_sample_offsets, n_frames, params, bin_len, d_levels, n_bins,
                             d_frame_status=None, d_seg_index=None, seg_blocks=0, tones=None):
        """x3_tone_bank_levels_dev: len(tones) planes of n_bins x3_tone_level records (TONE_DTYPE), plane t what
        tone_levels_dev writes for tones[t], in one pass over the stream (tones: 1 .. TONE_BANK_MAX Tone, or a
        LevelToneBank as it is); asynchronous, levels_result waits"""
        return lib().x3_tone_bank_levels_dev(self._h, d_x3, x3_len, d_frame_offsets, d_sample_offsets, n_frames, C.byref(params),
                                             d_seg_index, seg_blocks, bin_len, d_levels, n_bins, d_frame_status,
                                             self._tone_bank_arg(tones))

    def corpus_tone_bank_levels_dev(self, corpus, bin_len, d_levels, n_rows, d_frame_status=None, tones=None):
        """x3_corpus_tone_bank_levels_dev: len(tones) planes of corpus_tone_levels_dev's n_rows records, every entry at phase
        0 in every plane; asynchronous, levels_result waits"""
        return lib().x3_corpus_tone_bank_levels_dev(self._h, corpus._h, bin_len, d_levels, n_rows, d_frame_status,
                                                    self._tone_bank_arg(tones))

    def tone_power_levels_dev(self, d_tone, n_rows, d_levels):
        """x3_tone_power_levels_dev: n_rows tone records -> the x3_level records of the band's level (d_levels == d_tone: in
        place); asynchronous on the context's stream, no result call"""
        return lib().x3_tone_power_levels_dev(self._h, d_tone, n_rows, d_levels)

    def levels_result(self):
        """-> (rc, n_bad_frames, first_bad, first_bad_status) of the last levels_dev / corpus_levels_dev"""
        nb, fb, st = C.c_uint64(0), C.c_uint64(0), C.c_int32(0)
        rc = lib().x3_levels_result(self._h, C.byref(nb), C.byref(fb), C.byref(st))
        return rc, nb.value, fb.value, st.value

    def corpus_levels_dev(self, corpus, bin_len, d_levels, n_rows, d_frame_status=None):
        """x3_corpus_levels_dev: the levels of every entry of `corpus` (a Corpus), rows as Corpus.levels_rows; asynchronous"""
        return lib().x3_corpus_levels_dev(self._h, corpus._h, bin_len, d_levels, n_rows, d_frame_status)

    def events_dev(self, d_levels, n_bins, bin_len, d_total, rule, d_starts, d_lens, d_event_levels, cap, d_count):
        """x3_events_dev: runs of hot bins of n_bins level records (rule: an EventRule) as cap slots of (start u64, len u32,
        merged x3_level or None), the number found to d_count (u64); d_total: device pointer to the sample count; asynchronous"""
        return lib().x3_events_dev(self._h, d_levels, n_bins, bin_len, d_total, C.byref(rule), d_starts, d_lens, d_event_levels,
                                   cap, d_count)

    def corpus_events_dev(self, corpus, d_levels, n_rows, bin_len, rule, d_entries, d_starts, d_lens, d_event_levels, cap,
                          d_count):
        """x3_corpus_events_dev: the same over the rows of Context.corpus_levels_dev, d_entries (u32) as well; asynchronous"""
        return lib().x3_corpus_events_dev(self._h, corpus._h, d_levels, n_rows, bin_len, C.byref(rule), d_entries, d_starts,
                                          d_lens, d_event_levels, cap, d_count)

    def events_result(self):
        """-> (rc, count) of the last events_dev / corpus_events_dev: the events found (may exceed the call's cap)"""
        n = C.c_uint64(0)
        rc = lib().x3_events_result(self._h, C.byref(n))
        return rc, n.value

    def level_quantiles_dev(self, d_levels, n_bins, bin_len, d_total, key, q_ppm, d_values, d_counted):
        """x3_level_quantiles_dev: the quantiles q_ppm (millionths, 1 .. 8 of them) of the keys (LEVEL_KEY_PEAK /
        LEVEL_KEY_MEAN_SQ) of n_bins level records into d_values (u32 [len(q_ppm)]) and K into d_counted (u32);
        asynchronous -> rc"""
        q = (C.c_uint32 * len(q_ppm))(*q_ppm)
        return lib().x3_level_quantiles_dev(self._h, d_levels, n_bins, bin_len, d_total, key, q, len(q_ppm), d_values, d_counted)

    def corpus_level_quantiles_dev(self, corpus, d_levels, n_rows, bin_len, key, q_ppm, d_values, d_counted):
        """x3_corpus_level_quantiles_dev: the same per entry over the rows of corpus_levels_dev: d_values u32
        [n_entries * len(q_ppm)], d_counted u32 [n_entries]; asynchronous"""
        q = (C.c_uint32 * len(q_ppm))(*q_ppm)
        return lib().x3_corpus_level_quantiles_dev(self._h, corpus._h, d_levels, n_rows, bin_len, key, q, len(q_ppm), d_values,
                                                   d_counted)

    def level_quantiles_result(self):
        """-> (rc, n_empty, first_empty) of the last quantiles or thresholds call: entries without a counting row, the first
        of them (the entry count if none)"""
        a, b = C.c_uint64(0), C.c_uint64(0)
        rc = lib().x3_level_quantiles_result(self._h, C.byref(a), C.byref(b))
        return rc, a.value, b.value

    def level_thresholds_dev(self, d_levels, n_bins, bin_len, d_total, threshold_rule, d_thr):
        """x3_level_thresholds_dev: one EVENT_THRESHOLD_DTYPE record from the quantiles a ThresholdRule names; asynchronous;
        level_quantiles_result waits"""
        return lib().x3_level_thresholds_dev(self._h, d_levels, n_bins, bin_len, d_total, C.byref(threshold_rule), d_thr)

    def corpus_level_thresholds_dev(self, corpus, d_levels, n_rows, bin_len, threshold_rule, d_thr):
        """x3_corpus_level_thresholds_dev: a record per entry; asynchronous"""
        return lib().x3_corpus_level_thresholds_dev(self._h, corpus._h, d_levels, n_rows, bin_len, C.byref(threshold_rule), d_thr)

    def events_adaptive_dev(self, d_levels, n_bins, bin_len, d_total, rule, d_thr, d_starts, d_lens, d_event_levels, cap, d_count):
        """x3_events_adaptive_dev: events_dev with the rule's two values (both 0 in `rule`) taken from the record at d_thr;
        asynchronous; events_result waits"""
        return lib().x3_events_adaptive_dev(self._h, d_levels, n_bins, bin_len, d_total, C.byref(rule), d_thr, d_starts, d_lens,
                                            d_event_levels, cap, d_count)

    def corpus_events_adaptive_dev(self, corpus, d_levels, n_rows, bin_len, rule, d_thr, d_entries, d_starts, d_lens,
                                   d_event_levels, cap, d_count):
        """x3_corpus_events_adaptive_dev: corpus_events_dev with the thresholds of entry e at d_thr[e]; asynchronous"""
        return lib().x3_corpus_events_adaptive_dev(self._h, corpus._h, d_levels, n_rows, bin_len, C.byref(rule), d_thr, d_entries,
                                                   d_starts, d_lens, d_event_levels, cap, d_count)

    def plane_events_dev(self, d_levels, plane_stride, n_bins, bin_len, d_total, rule, d_thr, d_starts, d_lens, d_event_planes,
                         d_event_levels, cap, d_count):
        """x3_plane_events_dev: the runs of bins loud in at least rule.min_planes of rule.n_planes planes of n_bins level
        records (plane t at d_levels + t * plane_stride records; rule: a PlaneEventRule) as cap slots of (start u64, len u32,
        mask of the planes loud in the event u32 or None, merged x3_level [n_planes, cap] or None); d_thr: None, or the
        EVENT_THRESHOLD_DTYPE record of every plane (then the rule has no values); asynchronous; events_result waits"""
        return lib().x3_plane_events_dev(self._h, d_levels, plane_stride, n_bins, bin_len, d_total, C.byref(rule), d_thr, d_starts,
                                         d_lens, d_event_planes, d_event_levels, cap, d_count)

    def corpus_plane_events_dev(self, corpus, d_levels, plane_stride, n_rows, bin_len, rule, d_thr, d_entries, d_starts, d_lens,
                                d_event_planes, d_event_levels, cap, d_count):
        """x3_corpus_plane_events_dev: the same over planes of the rows of Context.corpus_levels_dev, d_entries (u32) as well;
        d_thr: None, or records [n_planes, n_entries]; asynchronous"""
        return lib().x3_corpus_plane_events_dev(self._h, corpus._h, d_levels, plane_stride, n_rows, bin_len, C.byref(rule), d_thr,
                                                d_entries, d_starts, d_lens, d_event_planes, d_event_levels, cap, d_count)

    def range_levels_dev(self, d_x3, x3_len, d_frame_offsets, d_sample_offsets, n_frames, params, d_starts, d_lens, n_ranges,
                         bin_len, row_stride, d_levels, rows_cap, d_row_offsets, d_status, d_seg_index=None, seg_blocks=0):
        """x3_range_levels_dev: the x3_level records of range w = [d_starts[w], d_starts[w] + d_lens[w]), bins of bin_len
        positions from the range's start (0: one bin), rows packed (row_stride 0) or padded; asynchronous"""
        return lib().x3_range_levels_dev(self._h, d_x3, x3_len, d_frame_offsets, d_sample_offsets, n_frames, C.byref(params),
                                         d_seg_index, seg_blocks, d_starts, d_lens, n_ranges, bin_len, row_stride, d_levels,
                                         rows_cap, d_row_offsets, d_status)

    def corpus_range_levels_dev(self, corpus, d_entries, d_starts, d_lens, n_ranges, bin_len, row_stride, d_levels, rows_cap,
                                d_row_offsets, d_status):
        """x3_corpus_range_levels_dev: the same for ranges of entry d_entries[w] of `corpus` (a Corpus); asynchronous"""
        return lib().x3_corpus_range_levels_dev(self._h, corpus._h, d_entries, d_starts, d_lens, n_ranges, bin_len, row_stride,
                                                d_levels, rows_cap, d_row_offsets, d_status)

    def signal_range_levels_dev(self, d_x3, x3_len, d_frame_offsets, d_sample_offsets, n_frames, params, d_starts, d_lens,
                                n_ranges, bin_len, row_stride, d_levels, rows_cap, d_row_offsets, d_status, d_seg_index=None,
                                seg_blocks=0, signal=LEVEL_SIGNAL_SAMPLES):
        """x3_signal_range_levels_dev: range_levels_dev of the samples (LEVEL_SIGNAL_SAMPLES) or of the stream's first
        difference cut to the ranges (LEVEL_SIGNAL_DIFF); asynchronous, range_levels_result waits"""
        return lib().x3_signal_range_levels_dev(self._h, d_x3, x3_len, d_frame_offsets, d_sample_offsets, n_frames,
                                                C.byref(params), d_seg_index, seg_blocks, d_starts, d_lens, n_ranges, bin_len,
                                                row_stride, d_levels, rows_cap, d_row_offsets, d_status, signal)

    def corpus_signal_range_levels_dev(self, corpus, d_entries, d_starts, d_lens, n_ranges, bin_len, row_stride, d_levels,
                                       rows_cap, d_row_offsets, d_status, signal=LEVEL_SIGNAL_SAMPLES):
        """x3_corpus_signal_range_levels_dev: corpus_range_levels_dev with a signal; asynchronous"""
        return lib().x3_corpus_signal_range_levels_dev(self._h, corpus._h, d_entries, d_starts, d_lens, n_ranges, bin_len,
                                                       row_stride, d_levels, rows_cap, d_row_offsets, d_status, signal)

    def fir_range_levels_dev(self, d_x3, x3_len, d_frame_offsets, d_sample_offsets, n_frames, params, d_starts, d_lens,
                             n_ranges, bin_len, row_stride, d_levels, rows_cap, d_row_offsets, d_status, d_seg_index=None,
                             seg_blocks=0, fir=None):
        """x3_fir_range_levels_dev: range_levels_dev of the stream's FIR signal (fir: a Fir, or a LevelFir as it is) cut to
        the ranges; asynchronous, range_levels_result waits"""
        return lib().x3_fir_range_levels_dev(self._h, d_x3, x3_len, d_frame_offsets, d_sample_offsets, n_frames,
                                             C.byref(params), d_seg_index, seg_blocks, d_starts, d_lens, n_ranges, bin_len,
                                             row_stride, d_levels, rows_cap, d_row_offsets, d_status, self._fir_arg(fir))

    def corpus_fir_range_levels_dev(self, corpus, d_entries, d_starts, d_lens, n_ranges, bin_len, row_stride, d_levels,
                                    rows_cap, d_row_offsets, d_status, fir=None):
        """x3_corpus_fir_range_levels_dev: corpus_range_levels_dev of each entry's FIR signal; asynchronous"""
        return lib().x3_corpus_fir_range_levels_dev(self._h, corpus._h, d_entries, d_starts, d_lens, n_ranges, bin_len,
                                                    row_stride, d_levels, rows_cap, d_row_offsets, d_status, self._fir_arg(fir))

    def tone_range_levels_dev(self, d_x3, x3_len, d_frame_offsets, d_sample_offsets, n_frames, params, d_starts, d_lens,
                              n_ranges, bin_len, row_stride, d_levels, rows_cap, d_row_offsets, d_status, d_seg_index=None,
                              seg_blocks=0, tone=None):
        """x3_tone_range_levels_dev: range_levels_dev with x3_tone_level records (TONE_DTYPE), the stream's tone signal
        (tone: a Tone, or a LevelTone as it is) cut to the ranges -- the phase is the stream's, not the range's;
        asynchronous, range_levels_result waits"""
        return lib().x3_tone_range_levels_dev(self._h, d_x3, x3_len, d_frame_offsets, d_sample_offsets, n_frames,
                                              C.byref(params), d_seg_index, seg_blocks, d_starts, d_lens, n_ranges, bin_len,
                                              row_stride, d_levels, rows_cap, d_row_offsets, d_status, self._tone_arg(tone))

    def corpus_tone_range_levels_dev(self, corpus, d_entries, d_starts, d_lens, n_ranges, bin_len, row_stride, d_levels,
                                     rows_cap, d_row_offsets, d_status, tone=None):
        """x3_corpus_tone_range_levels_dev: corpus_range_levels_dev with tone records, the phase 0 at every entry's first
        position; asynchronous"""
        return lib().x3_corpus_tone_range_levels_dev(self._h, corpus._h, d_entries, d_starts, d_lens, n_ranges, bin_len,
                                                     row_stride, d_levels, rows_cap, d_row_offsets, d_status, self._tone_arg(tone))

    def tone_bank_range_levels_dev(self, d_x3, x3_len, d_frame_offsets, d_sample_offsets, n_frames, params, d_starts, d_lens,
                                   n_ranges, bin_len, row_stride, d_levels, rows_cap, d_row_offsets, d_status, d_seg_index=None,
                                   seg_blocks=0, tones=None):
        """x3_tone_bank_range_levels_dev: len(tones) planes of rows_cap x3_tone_level records (TONE_DTYPE), plane t -- at
        d_levels + t * rows_cap -- what tone_range_levels_dev writes for tones[t], in one pass over the covering frames
        (tones: 1 .. TONE_BANK_MAX Tone, or a LevelToneBank as it is); row offsets, statuses and the result are the single
        call's; asynchronous, range_levels_result waits"""
        return lib().x3_tone_bank_range_levels_dev(self._h, d_x3, x3_len, d_frame_offsets, d_sample_offsets, n_frames,
                                                   C.byref(params), d_seg_index, seg_blocks, d_starts, d_lens, n_ranges, bin_len,
                                                   row_stride, d_levels, rows_cap, d_row_offsets, d_status,
                                                   self._tone_bank_arg(tones))

    def corpus_tone_bank_range_levels_dev(self, corpus, d_entries, d_starts, d_lens, n_ranges, bin_len, row_stride, d_levels,
                                          rows_cap, d_row_offsets, d_status, tones=None):
        """x3_corpus_tone_bank_range_levels_dev: len(tones) planes of corpus_tone_range_levels_dev's rows_cap records, the
        phase 0 at every entry's first position in every plane; asynchronous"""
        return lib().x3_corpus_tone_bank_range_levels_dev(self._h, corpus._h, d_entries, d_starts, d_lens, n_ranges, bin_len,
                                                          row_stride, d_levels, rows_cap, d_row_offsets, d_status,
                                                          self._tone_bank_arg(tones))

    def range_levels_result(self):
        """-> (rc, n_bad, first_bad, first_bad_status, total_rows) of the last range_levels_dev / corpus_range_levels_dev"""
        nb, fb, st, tot = C.c_uint64(0), C.c_uint64(0), C.c_int32(0), C.c_uint64(0)
        rc = lib().x3_range_levels_result(self._h, C.byref(nb), C.byref(fb), C.byref(st), C.byref(tot))
        return rc, nb.value, fb.value, st.value, tot.value

    def spectra_rows_dev(self, d_samples, samples_cap, d_offsets, d_lens, d_in_status, n_ranges, rule, row_stride, d_out,
                         rows_cap, d_row_offsets, d_status):
        """x3_spectra_rows_dev: the exact integer STFT (rule: a SpectraRule, None: NULL, which the library refuses) of the
        int16 rows d_lens[w] samples at d_samples + d_offsets[w], as decode_ranges_dev / Corpus.ranges_into wrote them;
        d_in_status: that call's statuses or None, may equal d_status; row_stride 0: packed rows at d_row_offsets[w], else
        rows at w * row_stride; d_out: rows_cap rows of B = n_fft / 2 + 1 (re, im) int64 pairs (SPECTRA_SUMS) or uint32
        powers (SPECTRA_POWER); asynchronous, spectra_result waits"""
        return lib().x3_spectra_rows_dev(self._h, d_samples, samples_cap, d_offsets, d_lens, d_in_status, n_ranges,
                                         C.byref(rule) if rule is not None else None, row_stride, d_out, rows_cap,
                                         d_row_offsets, d_status)

    def spectra_levels_dev(self, d_samples, samples_cap, d_offsets, d_lens, d_in_status, n_ranges, rule, fold, row_stride,
                           d_levels, rows_cap, d_row_offsets, d_status):
        """x3_spectra_levels_dev: spectra_rows_dev's POWER words (rule: a SpectraRule with SPECTRA_POWER) folded by fold (a
        SpectraFold; None: NULL, which the library refuses) into bands and time bins of frames_per_bin frames, as n_bands
        planes of x3_level records at d_levels + b * plane_stride records; the rows are the time bins, laid as
        spectra_rows_dev lays its rows; asynchronous, spectra_result waits (total_rows: the time bins)"""
        return lib().x3_spectra_levels_dev(self._h, d_samples, samples_cap, d_offsets, d_lens, d_in_status, n_ranges,
                                           C.byref(rule) if rule is not None else None,
                                           C.byref(fold) if fold is not None else None, row_stride, d_levels, rows_cap,
                                           d_row_offsets, d_status)

    def spectra_result(self):
        """-> (rc, n_bad, first_bad, first_bad_status, total_rows) of the last spectra_rows_dev / spectra_levels_dev"""
        nb, fb, st, tot = C.c_uint64(0), C.c_uint64(0), C.c_int32(0), C.c_uint64(0)
        rc = lib().x3_spectra_result(self._h, C.byref(nb), C.byref(fb), C.byref(st), C.byref(tot))
        return rc, nb.value, fb.value, st.value, tot.value

    def decode_streams_dev(self, d_x3, x3_len, offsets, lengths, params, d_out, row_len, out_format, d_results, flags=0):
        """x3_decode_streams_dev: entry s = bytes [offsets[s], offsets[s] + lengths[s]) of d_x3 -> row s of d_out
        (len(offsets) x row_len samples) and d_results[s] (asynchronous; offsets / lengths: host sequences)"""
        offs = np.ascontiguousarray(offsets, dtype=np.uint64)
        lens = np.ascontiguousarray(lengths, dtype=np.uint64)
        if offs.size != lens.size:
            raise ValueError("offsets and lengths differ in length")
        return lib().x3_decode_streams_dev(self._h, d_x3, x3_len, offs.ctypes.data, lens.ctypes.data, offs.size, flags,
                                           C.byref(params), d_out, row_len, out_format, d_results)

    def decode_streams_result(self):
        """-> (rc, n_bad, first_bad, first_bad_status) of the last decode_streams_dev"""
        nb, fb, st = C.c_uint64(0), C.c_uint64(0), C.c_int(0)
        rc = lib().x3_decode_streams_result(self._h, C.byref(nb), C.byref(fb), C.byref(st))
        return rc, nb.value, fb.value, st.value

    def synth_dev(self, kind, seed, start, n, d_out):
        rc = lib().x3_synth_dev(self._h, kind, seed, start, n, d_out)
        if rc:
            raise X3Error(rc, "x3_synth_dev: " + self.last_error())

    def enable_kernel_timing(self, on=True):
        lib().x3_ctx_enable_kernel_timing(self._h, 1 if on else 0)

    def reset_kernel_time(self):
        lib().x3_ctx_reset_kernel_time(self._h)

    def kernel_time(self, which):
        ms, cnt = C.c_double(0), C.c_uint64(0)
        rc = lib().x3_ctx_kernel_time(self._h, which, C.byref(ms), C.byref(cnt))
        if rc:
            raise X3Error(rc, "x3_ctx_kernel_time")
        return ms.value, cnt.value

    def kernel_times(self, which):
        """every timed launch's own time in ms, oldest first"""
        n = C.c_uint64(0)
        lib().x3_ctx_kernel_times(self._h, which, None, 0, C.byref(n))
        out = (C.c_double * max(1, n.value))()
        rc = lib().x3_ctx_kernel_times(self._h, which, out, n.value, C.byref(n))
        if rc:
            raise X3Error(rc, "x3_ctx_kernel_times")
        return [out[i] for i in range(n.value)]

    def launch_log(self, which):
        """the kernels' own launch log (x3_ctx_launch_log): list of dicts, oldest first"""
        n = C.c_uint64(0)
        out = (C.c_uint32 * (4 * 256))()
        rc = lib().x3_ctx_launch_log(self._h, which, out, 256, C.byref(n))
        if rc:
            raise X3Error(rc, "x3_ctx_launch_log")
        return [{"target_ticks16": out[4 * i], "achieved_ticks16": out[4 * i + 1], "clock_mhz": out[4 * i + 2] / 1000.0,
                 "life_us": out[4 * i + 3] / 100.0} for i in range(min(n.value, 256))]

    def alloc(self, nbytes):
        p = C.c_void_p()
        rc = lib().x3_dev_alloc(self._h, nbytes, C.byref(p))
        if rc:
            raise X3Error(rc, "x3_dev_alloc: " + self.last_error())
        return p.value

    def free(self, ptr):
        lib().x3_dev_free(self._h, ptr)

    def upload(self, d_dst, arr):
        arr = np.ascontiguousarray(arr)
        rc = lib().x3_dev_upload(self._h, d_dst, arr.ctypes.data, arr.nbytes)
        if rc:
            raise X3Error(rc, "x3_dev_upload: " + self.last_error())

    def download(self, d_src, nbytes, dtype=np.uint8):
        out = np.empty(nbytes // np.dtype(dtype).itemsize, dtype=dtype)
        rc = lib().x3_dev_download(self._h, out.ctypes.data, d_src, nbytes)
        if rc:
            raise X3Error(rc, "x3_dev_download: " + self.last_error())
        return out


def _ranges_torch(ctx, enqueue, what, starts, lens, padded_to, capacity, dtype, entries=None):
    """The torch side of WindowSource.ranges / Corpus.ranges: device tensors in, (out, offsets, status) device tensors out.
    enqueue(d_entries, d_starts, d_lens, n, stride, d_out, cap, fmt, d_off, d_status) -> rc."""
    import torch
    if dtype not in (torch.int16, torch.float32):
        raise ValueError("dtype: torch.int16 or torch.float32")
    dev = torch.device("cuda", torch.cuda.current_device())

    def on_dev(a, dt):   # (unsigned words travel as the signed tensors of the same bits: torch's unsigned types do little)
        signed = {np.uint64: torch.int64, np.uint32: torch.int32}[dt]
        if not isinstance(a, torch.Tensor):
            a = torch.from_numpy(np.ascontiguousarray(a, dtype=dt).view(np.int64 if dt is np.uint64 else np.int32))
        elif a.dtype.itemsize == signed.itemsize and not a.dtype.is_floating_point:
            a = a.view(signed)
        else:
            a = a.to(signed)
        return a.to(dev).contiguous()
    starts, lens = on_dev(starts, np.uint64), on_dev(lens, np.uint32)
    n = starts.numel()
    if starts.dim() != 1 or lens.shape != starts.shape or n == 0:
        raise ValueError("starts and lens: 1-D, non-empty, of one length")
    d_ent = None
    if entries is not None:
        entries = on_dev(entries, np.uint32)
        if entries.shape != starts.shape:
            raise ValueError("entries: as many as starts")
        d_ent = entries.data_ptr()
    if padded_to is not None:
        if padded_to <= 0:
            raise ValueError("padded_to: a positive row stride")
        stride, cap = int(padded_to), n * int(padded_to)
        out = torch.empty((n, stride), dtype=dtype, device=dev)
    else:
        stride = 0
        cap = int(capacity) if capacity is not None else int((lens.to(torch.int64) & 0xFFFFFFFF).sum().item())   # (the one host trip)
        out = torch.empty(max(cap, 1), dtype=dtype, device=dev)
    offsets = torch.empty(n + 1, dtype=torch.int64, device=dev)   # (below 2^63: n < 2^31 lengths of 32 bits)
    status = torch.empty(n, dtype=torch.int32, device=dev)
    torch.cuda.current_stream().synchronize()    # (the context's stream is not torch's: the inputs are ready from here)
    rc = enqueue(d_ent, starts.data_ptr(), lens.data_ptr(), n, stride, out.data_ptr(), cap,
                 WINDOW_F32 if dtype == torch.float32 else WINDOW_I16, offsets.data_ptr(), status.data_ptr())
    if rc:
        raise X3Error(rc, what + ": " + ctx.last_error())
    rc = ctx.decode_ranges_result()[0]
    if rc:
        raise X3Error(rc, "x3_decode_ranges_result: " + ctx.last_error())
    return out[:cap] if padded_to is None else out, offsets, status


class _BandFold:
    """What the range_band_levels forms hand to _range_spectra_torch: frames_per_bin and bands as the caller gave them; and,
    WindowSource.band_levels' only, `into` = (planes uint8 [K, R, 32] on the device, first row) -- the records go to rows
    [first row, first row + capacity) of those planes, plane stride R -- and `device_map` = (the int32 tensor of the band map on
    the device, K) in the place of bands"""
    __slots__ = ("frames_per_bin", "bands", "into", "device_map")

    def __init__(self, frames_per_bin, bands, into=None, device_map=None):
        self.frames_per_bin, self.bands, self.into, self.device_map = int(frames_per_bin), bands, into, device_map


def _range_spectra_torch(ctx, enqueue, what, starts, lens, n_fft, hop, power, table, padded_to, capacity, sample_capacity,
                         entries=None, fold=None):
    """The torch side of WindowSource.range_spectra / Corpus.range_spectra: the ranges call (packed int16) and the spectra
    call behind it on the context's stream, no wait and no host trip in between -> (spectra, row_offsets, status, samples,
    sample_offsets) device tensors.  enqueue(d_entries, d_starts, d_lens, n, rule, d_samples, samples_cap, d_sample_offsets,
    stride, d_out, rows_cap, d_row_offsets, d_status, fold=None) -> (rc of the ranges call, rc of the spectra call or None).
    fold (the range_band_levels forms): a _BandFold -- the rows are time bins of fold.frames_per_bin frames, the output is
    levels uint8 [K, rows, 32], enqueue gets the SpectraFold made from it as `fold`, and -> (levels, row_offsets, status)."""
    import torch
    dev = torch.device("cuda", torch.cuda.current_device())
    n_fft = int(n_fft)
    hop = n_fft if hop is None else int(hop)
    if n_fft not in SPECTRA_NFFTS or not 1 <= hop <= 0x7FFFFFFF:
        raise ValueError("n_fft: one of %s; hop: 1 .. 2^31 - 1" % (SPECTRA_NFFTS,))
    per_bin = 1
    if fold is not None:
        per_bin = fold.frames_per_bin
        if not 1 <= per_bin <= 0x7FFFFFFF:
            raise ValueError("frames_per_bin: 1 .. 2^31 - 1")
        if fold.device_map is not None:
            bin_band, n_bands = fold.device_map  # (band_levels: the map is on the device already, with its K)
        else:
            m, n_bands = spectra_bin_band(n_fft, fold.bands)
            bin_band = torch.from_numpy(m.view(np.int32)).to(dev)

    def on_dev(a, dt):   # (as in _ranges_torch: unsigned words travel as the signed tensors of the same bits)
        signed = {np.uint64: torch.int64, np.uint32: torch.int32}[dt]
        if not isinstance(a, torch.Tensor):
            a = torch.from_numpy(np.ascontiguousarray(a, dtype=dt).view(np.int64 if dt is np.uint64 else np.int32))
        elif a.dtype.itemsize == signed.itemsize and not a.dtype.is_floating_point:
            a = a.view(signed)
        else:
            a = a.to(signed)
        return a.to(dev).contiguous()
    starts, lens = on_dev(starts, np.uint64), on_dev(lens, np.uint32)
    n = starts.numel()
    if starts.dim() != 1 or lens.shape != starts.shape or n == 0:
        raise ValueError("starts and lens: 1-D, non-empty, of one length")
    d_ent = None
    if entries is not None:
        entries = on_dev(entries, np.uint32)
        if entries.shape != starts.shape:
            raise ValueError("entries: as many as starts")
        d_ent = entries.data_ptr()
    if padded_to is not None and padded_to <= 0:
        raise ValueError("padded_to: a positive row stride")
    stride = int(padded_to) if padded_to is not None else 0
    rows_cap = n * stride if stride else (int(capacity) if capacity is not None else None)
    samples_cap = int(sample_capacity) if sample_capacity is not None else None
    if rows_cap is None or samples_cap is None:   # (the one host trip: the lengths; both sums come from them)
        ln = (lens.to(torch.int64) & 0xFFFFFFFF).cpu().numpy()
        if samples_cap is None:
            samples_cap = int(ln.sum())
        if rows_cap is None:
            rows_cap = int((-(-np.where(ln < n_fft, 0, (ln - n_fft) // hop + 1) // per_bin)).sum())
    if table is None:
        d_table = ctx.tone_table_dev()
    else:
        if not isinstance(table, torch.Tensor):
            table = torch.from_numpy(np.ascontiguousarray(table, dtype=np.int16))
        if table.dtype != torch.int16 or table.numel() != 2 * TONE_TABLE_PAIRS:
            raise ValueError("table: %d (cos, sin) int16 pairs" % TONE_TABLE_PAIRS)
        table = table.to(dev).contiguous()
        d_table = table.data_ptr()
    nb = n_fft // 2 + 1
    rule = SpectraRule(n_fft, hop, SPECTRA_POWER if power else SPECTRA_SUMS, 0, d_table)
    samples = torch.empty(max(samples_cap, 1), dtype=torch.int16, device=dev)
    sample_offsets = torch.empty(n + 1, dtype=torch.int64, device=dev)
    spectra = None if fold is not None else torch.empty((max(rows_cap, 1), nb) if power else (max(rows_cap, 1), nb, 2),
                                                        dtype=torch.int32 if power else torch.int64, device=dev)
    row_offsets = torch.empty(n + 1, dtype=torch.int64, device=dev)
    status = torch.empty(n, dtype=torch.int32, device=dev)
    c_fold = None
    if fold is not None:
        if fold.into is None:
            spectra = torch.empty((n_bands, max(rows_cap, 1), 32), dtype=torch.uint8, device=dev)
            d_out, plane_stride = spectra.data_ptr(), 0
        else:
            planes, first = fold.into
            if (planes.dtype != torch.uint8 or planes.dim() != 3 or planes.shape[0] != n_bands or planes.shape[2] != 32
                    or not planes.is_contiguous() or not 0 <= first <= planes.shape[1] - max(rows_cap, 1)):
                raise ValueError("into: contiguous uint8 planes [K, R, 32] with first + capacity <= R")
            spectra = planes
            d_out, plane_stride = planes.data_ptr() + 32 * first, planes.shape[1]
        c_fold = SpectraFold(per_bin, n_bands, plane_stride, bin_band.data_ptr(), 0)
    else:
        d_out = spectra.data_ptr()
    torch.cuda.current_stream().synchronize()    # (the context's stream is not torch's: the inputs are ready from here)
    rc, rc2 = enqueue(d_ent, starts.data_ptr(), lens.data_ptr(), n, rule, samples.data_ptr(), max(samples_cap, 1),
                      sample_offsets.data_ptr(), stride, d_out, max(rows_cap, 1), row_offsets.data_ptr(),
                      status.data_ptr(), **({} if c_fold is None else {"fold": c_fold}))
    if rc:
        raise X3Error(rc, what + ": " + ctx.last_error())
    rc = ctx.decode_ranges_result()[0]   # (waits for both: one stream)
    if rc:
        raise X3Error(rc, "x3_decode_ranges_result: " + ctx.last_error())
    if rc2:
        raise X3Error(rc2, ("x3_spectra_rows_dev: " if fold is None else "x3_spectra_levels_dev: ") + ctx.last_error())
    rc = ctx.spectra_result()[0]
    if rc:
        raise X3Error(rc, "x3_spectra_result: " + ctx.last_error())
    if fold is not None:
        return (spectra[:, :rows_cap] if fold.into is None else spectra), row_offsets, status
    return spectra[:rows_cap], row_offsets, status, samples[:samples_cap], sample_offsets


def _range_spectra_enqueue(ctx, ranges_into):
    """the enqueue of _range_spectra_torch and the body of the range_spectra_into / range_band_levels_into forms:
    ranges_into(d_starts-or-entries ..., packed int16) then x3_spectra_rows_dev -- or, with a SpectraFold as `fold`,
    x3_spectra_levels_dev -- in place on its statuses"""
    def enqueue(d_ent, d_starts, d_lens, n, rule, d_samples, samples_cap, d_sample_offsets, stride, d_out, rows_cap, d_row_offsets,
                d_status, fold=None):
        rc = ranges_into(d_ent, d_starts, d_lens, n, 0, d_samples, samples_cap, WINDOW_I16, d_sample_offsets, d_status)
        if rc:
            return rc, None
        if fold is not None:          # the range_band_levels forms
            return 0, ctx.spectra_levels_dev(d_samples, samples_cap, d_sample_offsets, d_lens, d_status, n, rule, fold, stride,
                                             d_out, rows_cap, d_row_offsets, d_status)
        return 0, ctx.spectra_rows_dev(d_samples, samples_cap, d_sample_offsets, d_lens, d_status, n, rule, stride, d_out, rows_cap,
                                       d_row_offsets, d_status)
    return enqueue


def _range_levels_torch(ctx, enqueue, what, starts, lens, bin_len, padded_to, capacity, entries=None, band=False, planes=None):
    """The torch side of WindowSource.range_levels / Corpus.range_levels: device tensors in, (levels uint8 [rows, 32],
    row_offsets int64 [n + 1], status int32 [n]) device tensors out (levels: see event_levels_view).
    enqueue(d_entries, d_starts, d_lens, n, bin_len, stride, d_levels, cap, d_off, d_status) -> rc.
    band (the tone calls): the records tensor is allocated zeroed and x3_tone_power_levels_dev runs in place over all of it
    behind the call -- a zero record has n == 0, which the adapter turns into the identity, so the records of ranges
    without room are defined too.
    planes (the tone bank calls): levels is uint8 [planes, rows, 32], so many planes of `rows` records with plane stride
    rows_cap = rows, and the adapter of band=True runs once over all planes * rows of them."""
    import torch
    dev = torch.device("cuda", torch.cuda.current_device())
    bin_len = int(bin_len)
    if bin_len < 0:
        raise ValueError("bin_len: 0 (one bin) or a positive bin length")

    def on_dev(a, dt):   # (as in _ranges_torch: unsigned words travel as the signed tensors of the same bits)
        signed = {np.uint64: torch.int64, np.uint32: torch.int32}[dt]
        if not isinstance(a, torch.Tensor):
            a = torch.from_numpy(np.ascontiguousarray(a, dtype=dt).view(np.int64 if dt is np.uint64 else np.int32))
        elif a.dtype.itemsize == signed.itemsize and not a.dtype.is_floating_point:
            a = a.view(signed)
        else:
            a = a.to(signed)
        return a.to(dev).contiguous()
    starts, lens = on_dev(starts, np.uint64), on_dev(lens, np.uint32)
    n = starts.numel()
    if starts.dim() != 1 or lens.shape != starts.shape or n == 0:
        raise ValueError("starts and lens: 1-D, non-empty, of one length")
    d_ent = None
    if entries is not None:
        entries = on_dev(entries, np.uint32)
        if entries.shape != starts.shape:
            raise ValueError("entries: as many as starts")
        d_ent = entries.data_ptr()
    if padded_to is not None:
        if padded_to <= 0:
            raise ValueError("padded_to: a positive row stride")
        stride, cap = int(padded_to), n * int(padded_to)
    else:
        stride = 0
        if capacity is not None:
            cap = int(capacity)
        elif bin_len == 0 or bin_len >= 1 << 32:   # (a length has 32 bits: one bin a range)
            cap = n
        else:   # (the one host trip: the sum of max(1, ceil(len / bin_len)))
            ln = lens.to(torch.int64) & 0xFFFFFFFF
            cap = int(torch.clamp((ln + (bin_len - 1)) // bin_len, min=1).sum().item())
    levels = (torch.zeros if band else torch.empty)((planes or 1, max(cap, 1), LEVEL_DTYPE.itemsize), dtype=torch.uint8, device=dev)
    offsets = torch.empty(n + 1, dtype=torch.int64, device=dev)
    status = torch.empty(n, dtype=torch.int32, device=dev)
    torch.cuda.current_stream().synchronize()    # (the context's stream is not torch's: the inputs are ready from here)
    rc = enqueue(d_ent, starts.data_ptr(), lens.data_ptr(), n, bin_len, stride, levels.data_ptr(), cap, offsets.data_ptr(),
                 status.data_ptr())
    if rc:
        raise X3Error(rc, what + ": " + ctx.last_error())
    if band and cap > 0:   # (behind the call on the context's stream, in front of the wait)
        rc = ctx.tone_power_levels_dev(levels.data_ptr(), (planes or 1) * cap, levels.data_ptr())
        if rc:
            raise X3Error(rc, "x3_tone_power_levels_dev: " + ctx.last_error())
    rc = ctx.range_levels_result()[0]
    if rc:
        raise X3Error(rc, "x3_range_levels_result: " + ctx.last_error())
    if band:
        ctx.sync()
    return (levels[:, :cap] if planes else levels[0, :cap]), offsets, status


def _level_quantiles_torch(ctx, n_rows, n_ent, n_q, enqueue_levels, enqueue_quantiles):
    """The torch side of level_quantiles of a WindowSource or a Corpus: the levels call and the quantiles call back
    to back -> (values int32 [n_ent, n_q], counted int32 [n_ent]) on the device (the bits of the uint32 words)."""
    import torch
    dev = torch.device("cuda", torch.cuda.current_device())
    levels = torch.empty((n_rows, LEVEL_DTYPE.itemsize), dtype=torch.uint8, device=dev)
    values = torch.empty((n_ent, n_q), dtype=torch.int32, device=dev)
    counted = torch.empty(n_ent, dtype=torch.int32, device=dev)
    torch.cuda.current_stream().synchronize()    # (the context's stream is not torch's)
    rc = enqueue_levels(levels.data_ptr(), n_rows)
    if rc:
        raise X3Error(rc, "levels: " + ctx.last_error())
    rc = enqueue_quantiles(levels.data_ptr(), values.data_ptr(), counted.data_ptr())
    if rc:
        ctx.levels_result()
        raise X3Error(rc, "level quantiles: " + ctx.last_error())
    rc = ctx.level_quantiles_result()[0] or ctx.levels_result()[0]
    if rc:
        raise X3Error(rc, "x3_level_quantiles_result: " + ctx.last_error())
    return values, counted


def _detect_torch(src, what, levels, n_planes, bin_len, capacity, enqueue_events, *, rule_planes=None, thresholds=None,
                  enqueue_levels=None, enqueue_thresholds=None, mask=True, sync=True, result_what=None):
    """The torch side of every detection call of src, a WindowSource or a Corpus: the chain levels (optional), thresholds
    (optional, per plane), events, enqueued back to back on the context's stream with no host trip in between.
    levels: a uint8 [K, rows, 32] device tensor of records of any origin, or None: K = n_planes planes of src's own rows
    that enqueue_levels(d_levels, n_rows) -> rc fills.  thresholds: None or a uint8 [K, n_entries, 16] device tensor;
    enqueue_thresholds(d_plane, n_rows, d_thr) -> rc, called per plane, fills one made here, which is then returned.
    enqueue_events(d_levels, n_rows, d_thr, d_entries, d_starts, d_lens, d_event_planes, d_event_levels, d_count) -> rc;
    d_entries is None for a WindowSource, d_event_planes without `mask`.  rule_planes: the planes the caller's rule is of.
    sync: wait for the context's stream behind the result calls.  An X3Error names `what`, or `result_what` where the events'
    or the levels' result call reports the failure.
    -> (([entries,] starts, lens, count), planes int32 [capacity] or None, event_levels uint8 [K, capacity, 32],
    thresholds or None): device tensors of `capacity` slots, count 0-d; the callers shape their tuples from it"""
    import torch
    ctx, with_entries = src.ctx, src._has_entries
    capacity = int(capacity)
    if capacity <= 0:
        raise ValueError("capacity: at least one slot")
    if not 0 < bin_len <= 0xFFFFFFFF:
        raise ValueError("bin_len: 1 .. 2^32 - 1")
    rec = LEVEL_DTYPE.itemsize
    if levels is None:
        dev = torch.device("cuda", torch.cuda.current_device())
        levels = torch.empty((n_planes, src._levels_rows(bin_len)[0], rec), dtype=torch.uint8, device=dev)
    elif not (isinstance(levels, torch.Tensor) and levels.is_cuda and levels.dtype == torch.uint8 and levels.dim() == 3 and
              1 <= levels.shape[0] <= EVENT_PLANES_MAX and levels.shape[1] > 0 and levels.shape[2] == rec):
        raise ValueError("levels: a uint8 tensor [K, rows, 32] on the device, K 1 .. %d" % EVENT_PLANES_MAX)
    elif levels.shape[1] != src._levels_rows(bin_len)[0]:   # (fewer would cut the detection short, more are never looked at)
        raise ValueError("levels: %d rows, but bins of %d positions over this source are %d rows"
                         % (levels.shape[1], bin_len, src._levels_rows(bin_len)[0]))
    levels = levels.contiguous()
    dev, k, n_rows = levels.device, levels.shape[0], levels.shape[1]
    if rule_planes is not None and rule_planes != k:
        raise ValueError("the rule is one of %d planes, the records have %d" % (rule_planes, k))
    n_ent = src.n_entries if with_entries else 1
    thr_rec = EVENT_THRESHOLD_DTYPE.itemsize
    if enqueue_thresholds is not None:
        thresholds = torch.empty((k, n_ent, thr_rec), dtype=torch.uint8, device=dev)
    elif thresholds is not None:
        if not (isinstance(thresholds, torch.Tensor) and thresholds.is_cuda and thresholds.dtype == torch.uint8 and
                tuple(thresholds.shape) == (k, n_ent, thr_rec)):
            raise ValueError("thresholds: a uint8 tensor [%d, %d, 16] on the device" % (k, n_ent))
        thresholds = thresholds.contiguous()
    entries = torch.empty(capacity, dtype=torch.int32, device=dev) if with_entries else None
    starts = torch.empty(capacity, dtype=torch.int64, device=dev)
    lens = torch.empty(capacity, dtype=torch.int32, device=dev)
    planes = torch.empty(capacity, dtype=torch.int32, device=dev) if mask else None
    event_levels = torch.empty((k, capacity, rec), dtype=torch.uint8, device=dev)
    count = torch.empty((), dtype=torch.int64, device=dev)
    torch.cuda.current_stream().synchronize()    # (the context's stream is not torch's)
    d_lv = levels.data_ptr()
    if enqueue_levels is not None:
        rc = enqueue_levels(d_lv, n_rows)
        if rc:
            raise X3Error(rc, "levels: " + ctx.last_error())
    rc = 0
    if enqueue_thresholds is not None:
        for t in range(k):       # (their pending slot is simply overwritten: one result call serves all K)
            rc = rc or enqueue_thresholds(d_lv + t * n_rows * rec, n_rows, thresholds.data_ptr() + t * n_ent * thr_rec)
    rc = rc or enqueue_events(d_lv, n_rows, thresholds.data_ptr() if thresholds is not None else None,
                              entries.data_ptr() if with_entries else None, starts.data_ptr(), lens.data_ptr(),
                              planes.data_ptr() if mask else None, event_levels.data_ptr(), count.data_ptr())
    # (every slot this call has made pending is read, whatever an earlier one said)
    r_ev = 0 if rc else ctx.events_result()[0]
    r_q = ctx.level_quantiles_result()[0] if enqueue_thresholds is not None else 0
    r_lv = ctx.levels_result()[0] if enqueue_levels is not None else 0
    if sync:
        ctx.sync()
    if rc or r_q:
        raise X3Error(rc or r_q, what + ": " + ctx.last_error())
    if r_ev or r_lv:
        raise X3Error(r_ev or r_lv, (result_what or what) + ": " + ctx.last_error())
    head = (starts, lens, count)
    return ((entries,) + head if with_entries else head), planes, event_levels, thresholds if enqueue_thresholds is not None else None


def _levels_np(src, what, bin_len, n_rows, dtype, enqueue, planes=None):
    """the host side of levels() / tone_levels() / tone_bank_levels() of src, a WindowSource or a Corpus: enqueue(d_levels,
    n_rows, d_status) -> rc, then the result and both downloads -> (records, frame statuses), a Corpus's row_first between
    them; n_rows: src's own count unless given; planes (tone_bank_levels): so many planes of n_rows records, returned as
    [planes, n_rows]"""
    ctx, n_frames = src.ctx, src.n_frames
    rows, rf = src._levels_rows(bin_len)
    if n_rows is None:
        n_rows = rows
    n_rec = n_rows * (planes or 1)
    d_lv, d_st = ctx.alloc(dtype.itemsize * n_rec), ctx.alloc(4 * max(n_frames, 1))
    try:
        rc = enqueue(d_lv, n_rows, d_st)
        if rc:
            raise X3Error(rc, what + ": " + ctx.last_error())
        rc = ctx.levels_result()[0]
        if rc:
            raise X3Error(rc, "x3_levels_result: " + ctx.last_error())
        st = ctx.download(d_st, 4 * n_frames, np.int32) if n_frames else np.zeros(0, dtype=np.int32)
        rec = ctx.download(d_lv, dtype.itemsize * n_rec, dtype)
        rec = rec.reshape(planes, n_rows) if planes else rec
        return (rec, st) if rf is None else (rec, rf, st)
    finally:
        for p in (d_lv, d_st):
            ctx.free(p)


def _levels_chain(src, bin_len, signal):
    """what events(), level_quantiles() and adaptive_events() of a WindowSource or a Corpus begin with -> (the rows of the
    levels of `signal`, enqueue_levels(d_levels, n_rows) -> rc)"""
    if not 0 < bin_len <= 0xFFFFFFFF:
        raise ValueError("bin_len: 1 .. 2^32 - 1")
    sig = level_signal(signal)
    n_rows = src._levels_rows(bin_len)[0]
    return n_rows, lambda d_lv, n: src.levels_into(bin_len, d_lv, n, None, sig)


def _bank_planes(tones):
    """the planes tone_bank_levels_into writes: tones as it takes them"""
    return tones.n_tones if isinstance(tones, LevelToneBank) else len(tone_bank(tones))


class _Detection:
    """The detection methods of WindowSource and Corpus, written once over what differs between the two: the rows of a bin
    length (_levels_rows), the entry count (n_entries; 1 where _has_entries is False), whether a call has an `entries`
    output (_has_entries: a Corpus's *_into enqueuers take d_entries in front of d_starts), and the *_into enqueuers
    themselves, which stay on each class.  All results are torch tensors on the device."""
    _has_entries = False

    def _ent(self, d_entries):
        return (d_entries,) if self._has_entries else ()

    def events(self, bin_len, rule, capacity, *, signal="samples"):
        """Levels (of `signal`, as in levels()) of bins of bin_len positions -- of every entry of a Corpus --, then the runs
        of hot bins under `rule` (an EventRule) as ranges, all on the device -> (starts int64 [capacity], lens int32
        [capacity], count 0-d int64, event_levels uint8 [capacity, 32]), a Corpus: entries int32 [capacity] in front.  Slots
        behind the events are zero-length ranges: ranges([entries,] starts, lens, padded_to=...) takes the tensors as they
        are.  count may exceed capacity: repeat with more."""
        _, enqueue_levels = _levels_chain(self, bin_len, signal)
        head, _, event_levels, _ = _detect_torch(
            self, "events", None, 1, bin_len, capacity,
            lambda d_lv, n, d_t, d_e, d_s, d_l, d_p, d_el, d_c: self.events_into(d_lv, n, bin_len, rule, *self._ent(d_e), d_s, d_l,
                                                                                 d_el, capacity, d_c),
            enqueue_levels=enqueue_levels, mask=False, sync=False, result_what="x3_events_result")
        return head + (event_levels[0],)

    def level_quantiles(self, bin_len, key, q_ppm, *, signal="samples"):
        """Levels (of `signal`, as in levels()) of bins of bin_len positions, then per entry the quantiles q_ppm (millionths)
        of their keys, on the device -> (values int32 [n_entries, len(q_ppm)], counted int32 [n_entries]); a WindowSource
        is one entry"""
        n_rows, enqueue_levels = _levels_chain(self, bin_len, signal)
        return _level_quantiles_torch(
            self.ctx, n_rows, self.n_entries if self._has_entries else 1, len(q_ppm), enqueue_levels,
            lambda d_lv, d_v, d_k: self.level_quantiles_into(d_lv, n_rows, bin_len, key, q_ppm, d_v, d_k))

    def adaptive_events(self, bin_len, threshold_rule, rule, capacity, *, signal="samples"):
        """events() with the rule's two values (both 0 in `rule`) chosen on the device, per entry, by `threshold_rule` (a
        ThresholdRule) -> what events() returns, and thresholds uint8 [n_entries, 16] (EVENT_THRESHOLD_DTYPE records; one
        for a WindowSource)"""
        _, enqueue_levels = _levels_chain(self, bin_len, signal)
        head, _, event_levels, thr = _detect_torch(
            self, "events", None, 1, bin_len, capacity,
            lambda d_lv, n, d_t, d_e, d_s, d_l, d_p, d_el, d_c: self.adaptive_events_into(d_lv, n, bin_len, rule, d_t,
                                                                                          *self._ent(d_e), d_s, d_l, d_el, capacity, d_c),
            enqueue_levels=enqueue_levels,
            enqueue_thresholds=lambda d_lv, n, d_t: self.level_thresholds_into(d_lv, n, bin_len, threshold_rule, d_t),
            mask=False, sync=False, result_what="x3_events_result")
        return head + (event_levels[0], thr[0])

    def _plane_events(self, levels, n_planes, bin_len, rule, capacity, **kw):
        head, planes, event_levels, thr = _detect_torch(
            self, "plane events", levels, n_planes, bin_len, capacity,
            lambda d_lv, n, d_t, d_e, d_s, d_l, d_p, d_el, d_c: self.plane_events_into(d_lv, n, n, bin_len, rule, d_t, *self._ent(d_e),
                                                                                      d_s, d_l, d_p, d_el, capacity, d_c),
            rule_planes=rule.n_planes, **kw)
        out = head + (planes, event_levels)
        return out if thr is None else out + (thr,)

    def plane_events(self, levels, bin_len, rule, capacity, *, thresholds=None):
        """The runs of bins that are loud in at least rule.min_planes of K planes of level records (levels: a uint8 torch
        tensor [K, rows, 32] on the device, records of any origin over this source's bins of bin_len positions -- exactly
        as many rows as cover the stream, or as levels() gives for a Corpus; anything else is a ValueError; rule: a
        PlaneEventRule; thresholds: None, or uint8 [K, n_entries, 16] records on the device, n_entries 1 for a WindowSource,
        and a rule without values) as ONE ordered, disjoint list of ranges; runs never cross an entry ->
        (starts int64 [capacity], lens int32 [capacity], count 0-d int64, planes int32 [capacity]: bit t set when plane t is
        loud in the event, event_levels uint8 [K, capacity, 32]) on the device, a Corpus: entries int32 [capacity] in front"""
        return self._plane_events(levels, None, bin_len, rule, capacity, thresholds=thresholds)

    def bank_events(self, bin_len, tones, rule, capacity):
        """tone_bank_levels_into(..., band=True), then plane_events over its planes, no wait in between -> as plane_events;
        tone_bank_range_levels([entries,] starts, lens, ...) takes the tensors as they are"""
        tones = tone_bank(tones)
        return self._plane_events(None, len(tones), bin_len, rule, capacity,
                                  enqueue_levels=lambda d_lv, n: self.tone_bank_levels_into(bin_len, tones, d_lv, n, band=True))

    def adaptive_bank_events(self, bin_len, tones, threshold_rule, rule, capacity):
        """bank_events with the two values of every plane of every entry (none in `rule`) chosen on the device by
        `threshold_rule` (a ThresholdRule), a thresholds call per plane in between -> as plane_events, and thresholds uint8
        [K, n_entries, 16] (n_entries 1 for a WindowSource)"""
        tones = tone_bank(tones)
        return self._plane_events(None, len(tones), bin_len, rule, capacity,
                                  enqueue_levels=lambda d_lv, n: self.tone_bank_levels_into(bin_len, tones, d_lv, n, band=True),
                                  enqueue_thresholds=lambda d_lv, n, d_t: self.level_thresholds_into(d_lv, n, bin_len,
                                                                                                     threshold_rule, d_t))


class WindowSource(_Detection):
    """Random access to one mono stream in HBM: windows of samples [start, start + length) as rows of a batch.

    `stream`: host bytes (uploaded once) or (d_x3, x3_len) of a device stream.  Without `frame_offsets` (a device pointer to
    n_frames + 1 byte offsets, with `n_frames`) the frames are found by x3_index_dev.  The sample offsets come from
    x3_sample_offsets_dev.  Without `seg_index` one is made once: index="decode" records it by a decode with
    x3_decode_dev_seg(record=1) (block length 20 and the default codes only; it decodes the whole stream into a buffer
    that is thrown away), index="walk" builds it with x3_seg_index_build_dev (any parameters, no sample buffer).  It is
    only ever a hint (seg_blocks=0: no index, frames decode whole)."""

    def __init__(self, ctx, stream, params=None, seg_blocks=32, frame_offsets=None, n_frames=None, seg_index=None,
                 index="decode"):
        if index not in ("decode", "walk"):
            raise ValueError('index: "decode" or "walk"')
        self.ctx, self.params, self.seg_blocks = ctx, params or Params.default(), seg_blocks
        self._own = []
        if isinstance(stream, tuple):
            self.d_x3, self.x3_len = stream
        else:
            b = np.ascontiguousarray(stream, dtype=np.uint8)
            self.x3_len = b.size
            self.d_x3 = self._alloc(max(b.size, 4))
            ctx.upload(self.d_x3, b)
        if frame_offsets is None:
            cap = self.x3_len // 20 + 2
            self.d_frame_offsets = self._alloc(8 * (cap + 1))
            d_wo = self._alloc(8 * cap)
            rc, nf, _, _ = ctx.index_dev(self.d_x3, self.x3_len, cap, self.d_frame_offsets, d_wo)
            if rc:
                raise X3Error(rc, "x3_index_dev: " + ctx.last_error())
            self.n_frames = nf
        else:
            self.d_frame_offsets, self.n_frames = frame_offsets, n_frames
        if not self.n_frames:
            raise X3Error(ERR_BAD_ARG, "WindowSource: the stream holds no frame")
        self.d_sample_offsets = self._alloc(8 * (self.n_frames + 1))
        rc = ctx.sample_offsets_dev(self.d_x3, self.x3_len, self.d_frame_offsets, self.n_frames, self.d_sample_offsets)
        if rc:
            raise X3Error(rc, "x3_sample_offsets_dev: " + ctx.last_error())
        self.total = int(ctx.download(self.d_sample_offsets + 8 * self.n_frames, 8, np.uint64)[0])
        self.d_seg_index = seg_index
        if seg_blocks and seg_index is None and lib().x3_seg_index_entries(self.n_frames, C.byref(self.params), seg_blocks):
            ne = lib().x3_seg_index_entries(self.n_frames, C.byref(self.params), seg_blocks)
            self.d_seg_index = self._alloc(8 * ne)
            if index == "walk":
                rc = ctx.seg_index_build_dev(self.d_x3, self.x3_len, self.d_frame_offsets, self.n_frames, self.params,
                                             self.d_seg_index, seg_blocks)
                if rc:
                    raise X3Error(rc, "x3_seg_index_build_dev: " + ctx.last_error())
                return
            ctx.upload(self.d_seg_index, np.zeros(ne, dtype=np.uint64))
            d_back = self._alloc(2 * max(self.total, 1))
            # (the three-wave decoder records the index; it takes caller offsets that are multiples of four samples)
            so = ctx.download(self.d_sample_offsets, 8 * self.n_frames, np.uint64)   # (where frames begin; not the total)
            x4 = ctx.get_option("wav_offsets_x4")
            ctx.set_option("wav_offsets_x4", 1 if not np.any(so & np.uint64(3)) else x4)
            try:
                rc = ctx.decode_dev_seg(self.d_x3, self.x3_len, self.d_frame_offsets, self.n_frames, self.params, d_back,
                                        self.total, self.d_seg_index, seg_blocks, record=True,
                                        d_wav_offsets=self.d_sample_offsets)
                if rc == 0:
                    ctx.decode_result()
            finally:
                ctx.set_option("wav_offsets_x4", x4)
                ctx.free(d_back)
                self._own.remove(d_back)
        if self.d_seg_index is None:
            self.seg_blocks = 0

    def _alloc(self, n):
        p = self.ctx.alloc(n)
        self._own.append(p)
        return p

    def decode_into(self, d_starts, n, length, d_out, fmt, d_status):
        """enqueue n windows (device pointers: d_starts n x u64, d_out n x length, d_status n x i32); -> rc"""
        return self.ctx.decode_windows_dev(self.d_x3, self.x3_len, self.d_frame_offsets, self.d_sample_offsets, self.n_frames,
                                           self.params, d_starts, n, length, d_out, fmt, d_status, self.d_seg_index,
                                           self.seg_blocks)

    def decode(self, starts, length, fmt=WINDOW_I16):
        """-> (rows np.int16 / np.float32 [n, length], statuses np.int32 [n])"""
        starts = np.ascontiguousarray(starts, dtype=np.uint64)
        n = starts.size
        esz = 4 if fmt == WINDOW_F32 else 2
        d_starts, d_out, d_st = self.ctx.alloc(8 * n), self.ctx.alloc(esz * n * length), self.ctx.alloc(4 * n)
        try:
            self.ctx.upload(d_starts, starts)
            rc = self.decode_into(d_starts, n, length, d_out, fmt, d_st)
            if rc:
                raise X3Error(rc, "x3_decode_windows_dev: " + self.ctx.last_error())
            rc = self.ctx.decode_windows_result()[0]
            if rc:
                raise X3Error(rc, "x3_decode_windows_result: " + self.ctx.last_error())
            rows = self.ctx.download(d_out, esz * n * length, np.float32 if fmt == WINDOW_F32 else np.int16)
            return rows.reshape(n, length), self.ctx.download(d_st, 4 * n, np.int32)
        finally:
            for p in (d_starts, d_out, d_st):
                self.ctx.free(p)

    def ranges_into(self, d_starts, d_lens, n, row_stride, d_out, out_cap, fmt, d_out_offsets, d_status):
        """enqueue n ranges (device pointers: d_starts n x u64, d_lens n x u32, d_out out_cap samples, d_out_offsets
        (n + 1) x u64 or None when padded, d_status n x i32); row_stride 0: packed; -> rc; decode_ranges_result waits"""
        return self.ctx.decode_ranges_dev(self.d_x3, self.x3_len, self.d_frame_offsets, self.d_sample_offsets, self.n_frames,
                                          self.params, d_starts, d_lens, n, row_stride, d_out, out_cap, fmt, d_out_offsets,
                                          d_status, self.d_seg_index, self.seg_blocks)

    def ranges(self, starts, lens, *, padded_to=None, capacity=None, dtype=None):
        """Variable-length windows [starts[w], starts[w] + lens[w]) -> (out, offsets, status), torch tensors on the device.
        starts / lens: torch tensors (device data stays on the device) or array-likes.  Packed (default): out is 1-D, range
        w at out[offsets[w]:offsets[w + 1]]; it holds `capacity` samples when given -- ranges without room are
        ERR_BAD_ARG, offsets[-1] tells what is needed -- and otherwise the sum of the lengths, which costs ONE
        synchronising sum on the host.  padded_to=S: out is [n, S], zeros behind each length, no host trip for sizes.
        dtype: torch.int16 (default) or torch.float32.  The call waits for its result (x3_decode_ranges_result)."""
        import torch
        return _ranges_torch(self.ctx, lambda e, *a: self.ranges_into(*a), "x3_decode_ranges_dev", starts, lens, padded_to,
                             capacity, dtype or torch.int16)

    def range_spectra_into(self, d_starts, d_lens, n, rule, d_samples, samples_cap, d_sample_offsets, row_stride, d_out, rows_cap,
                           d_row_offsets, d_status):
        """enqueue ranges_into (packed int16 into d_samples, offsets to d_sample_offsets) and, behind it with no wait,
        Context.spectra_rows_dev on those rows under rule (a SpectraRule), in place on d_status (device pointers)
        -> (rc of the ranges call, rc of the spectra call or None); decode_ranges_result and spectra_result wait"""
        return _range_spectra_enqueue(self.ctx, lambda e, *a: self.ranges_into(*a))(
            None, d_starts, d_lens, n, rule, d_samples, samples_cap, d_sample_offsets, row_stride, d_out, rows_cap, d_row_offsets,
            d_status)

    def range_spectra(self, starts, lens, n_fft, hop=None, *, power=True, table=None, padded_to=None, capacity=None,
                      sample_capacity=None):
        """The spectrogram of the ranges [starts[w], starts[w] + lens[w]): their samples (ranges(), packed int16) and, with
        no host trip in between, the exact integer STFT of every whole frame of n_fft samples at multiples of hop (None:
        n_fft) from each range's start (x3_spectra_rows_dev) -> (spectra, row_offsets, status, samples, sample_offsets),
        torch tensors on the device.  power=True: spectra is int32 [rows, n_fft / 2 + 1], the band power of every bin as
        the tone adapter forms it; False: int64 [rows, n_fft / 2 + 1, 2], the sums (re, im).  Range w's rows are
        spectra[row_offsets[w]:row_offsets[w + 1]] (packed; `capacity` rows when given), or begin at w * padded_to with
        zeros behind the range's last.  A range with a status (a damaged frame, no room) has rows of zeros only.  table:
        None for tone_table(), or 1 024 (cos, sin) int16 pairs.  Without capacity / sample_capacity the one host trip
        is the ranges' lengths.  The oscillator restarts at every frame, unlike tone_range_levels."""
        return _range_spectra_torch(self.ctx, _range_spectra_enqueue(self.ctx, lambda e, *a: self.ranges_into(*a)),
                                    "x3_decode_ranges_dev", starts, lens, n_fft, hop, power, table, padded_to, capacity,
                                    sample_capacity)

    def range_band_levels_into(self, d_starts, d_lens, n, rule, fold, d_samples, samples_cap, d_sample_offsets, row_stride,
                               d_levels, rows_cap, d_row_offsets, d_status):
        """range_spectra_into with Context.spectra_levels_dev behind the ranges call: rule a SpectraRule with SPECTRA_POWER,
        fold a SpectraFold, d_levels n_bands planes of x3_level records -> (rc of the ranges call, rc of the levels call or
        None); decode_ranges_result and spectra_result wait"""
        return _range_spectra_enqueue(self.ctx, lambda e, *a: self.ranges_into(*a))(
            None, d_starts, d_lens, n, rule, d_samples, samples_cap, d_sample_offsets, row_stride, d_levels, rows_cap,
            d_row_offsets, d_status, fold=fold)

    def range_band_levels(self, starts, lens, n_fft, hop=None, *, frames_per_bin=1, bands=None, table=None, padded_to=None,
                          capacity=None, sample_capacity=None):
        """Band levels of the ranges [starts[w], starts[w] + lens[w]): range_spectra's POWER words folded into bands and
        summed over frames_per_bin consecutive frames, with no row per frame stored (x3_spectra_levels_dev) -> (levels
        uint8 [K, rows, 32], row_offsets, status) on the device.  Range w's rows are its ceil(R / frames_per_bin) time
        bins (the last one possibly of fewer frames), in every plane at row_offsets[w] (packed; `capacity` rows when
        given) or w * padded_to with identity records behind them; plane b is band b.  A record (event_levels_view): n
        = the frames, sum_sq = the sum of the frames' band powers (each clamped to 2^30), max = -min = the peak of the
        loudest frame.  bands: None (one band per bin), K + 1 ascending bin edges (band_edges_third_octave gives some),
        or an array of n_fft / 2 + 1 band indices (spectra_bin_band).  A range with a status has identity records only.
        The planes go as they are into plane_events (eight at a time), events, level_quantiles and the thresholds."""
        return self._range_band_levels(starts, lens, n_fft, hop, _BandFold(frames_per_bin, bands), table, padded_to, capacity,
                                       sample_capacity)

    def _range_band_levels(self, starts, lens, n_fft, hop, fold, table, padded_to, capacity, sample_capacity):
        """range_band_levels and the chunks of band_levels; fold: a _BandFold"""
        return _range_spectra_torch(self.ctx, _range_spectra_enqueue(self.ctx, lambda e, *a: self.ranges_into(*a)),
                                    "x3_decode_ranges_dev", starts, lens, n_fft, hop, True, table, padded_to, capacity,
                                    sample_capacity, fold=fold)

    def band_levels(self, n_fft, hop=None, *, frames_per_bin, bands=None, table=None, chunk_samples=1 << 26, q=4):
        """Band levels of the whole stream -> levels uint8 [K, ceil(total / (frames_per_bin * hop)), 32] on the device (one
        identity row for a stream without a sample, as levels() gives one bin then):
        row i of plane b covers the positions [i * bin_len, (i + 1) * bin_len) with bin_len = frames_per_bin * hop and
        holds the frames that START there, n = frames_per_bin of them where they all fit into the stream; the trailing
        rows without a whole frame are the identity.  The planes go into plane_events(levels, bin_len, ...), events,
        level_quantiles and the thresholds as they are.
          Filled by a loop over chunks of ranges, the ranges' samples in a buffer of at most chunk_samples whatever the
        stream's length, one wait per chunk: range g begins at g * q * bin_len and is (q * frames_per_bin - 1) * hop +
        n_fft samples long (the last one cut at the stream's end), so it holds exactly the frames of q rows.  A DAMAGED
        FRAME of the stream therefore costs the q rows of every range that touches it -- they stay the identity -- where
        levels() loses only the samples of that frame; q is small for that reason.  hop > n_fft skips samples, as in
        range_spectra."""
        import torch
        n_fft = int(n_fft)
        hop = n_fft if hop is None else int(hop)
        per_bin, q = int(frames_per_bin), int(q)
        if n_fft not in SPECTRA_NFFTS or not 1 <= hop <= 0x7FFFFFFF or not 1 <= per_bin <= 0x7FFFFFFF or q < 1:
            raise ValueError("n_fft: one of %s; hop, frames_per_bin: 1 .. 2^31 - 1; q >= 1" % (SPECTRA_NFFTS,))
        bin_len = per_bin * hop
        range_len = (q * per_bin - 1) * hop + n_fft
        if range_len > 0xFFFFFFFF or range_len > chunk_samples:
            raise ValueError("a range of q * frames_per_bin frames (%d samples) does not fit chunk_samples" % range_len)
        dev = torch.device("cuda", torch.cuda.current_device())
        m, n_bands = spectra_bin_band(n_fft, bands)
        bin_band = torch.from_numpy(m.view(np.int32)).to(dev)
        rows = max(1, -(-self.total // bin_len))
        identity = np.frombuffer(np.array([(0, 0, 32767, -32768, 0, 0)], dtype=LEVEL_DTYPE).tobytes(), dtype=np.uint8).copy()
        planes = torch.from_numpy(identity).to(dev).expand(n_bands, rows, 32).contiguous()
        n_ranges = -(-self.total // (q * bin_len))
        per_chunk = max(1, int(chunk_samples) // range_len)
        for g0 in range(0, n_ranges, per_chunk):
            g = np.arange(g0, min(g0 + per_chunk, n_ranges), dtype=np.int64)
            starts = g * (q * bin_len)
            lens = np.minimum(range_len, self.total - starts)
            first = g0 * q
            cap = min(g.size * q, rows - first)     # (a range's rows: q, the last range's at most that)
            self._range_band_levels(starts, lens, n_fft, hop, _BandFold(per_bin, None, (planes, first), (bin_band, n_bands)),
                                    table, None,
                                    cap, int(lens.sum()))
        return planes

    def range_levels_into(self, d_starts, d_lens, n, bin_len, row_stride, d_levels, rows_cap, d_row_offsets, d_status,
                          signal=LEVEL_SIGNAL_SAMPLES):
        """enqueue the level records of n ranges (device pointers: d_starts n x u64, d_lens n x u32, d_levels rows_cap x
        x3_level, d_row_offsets (n + 1) x u64 or None when padded, d_status n x i32); row_stride 0: packed; signal: a
        LEVEL_SIGNAL_* value (a Fir or a Tone raises, "not built yet" on this keyword: fir_range_levels_into and
        tone_range_levels_into take them); -> rc;
        Context.range_levels_result waits"""
        if isinstance(signal, (Fir, Tone)):
            level_signal(signal, fir=False)
        return self.ctx.signal_range_levels_dev(self.d_x3, self.x3_len, self.d_frame_offsets, self.d_sample_offsets,
                                                self.n_frames, self.params, d_starts, d_lens, n, bin_len, row_stride, d_levels,
                                                rows_cap, d_row_offsets, d_status, self.d_seg_index, self.seg_blocks, signal)

    def range_levels(self, starts, lens, bin_len, *, padded_to=None, capacity=None, signal="samples"):
        """The x3_level records of the ranges [starts[w], starts[w] + lens[w]), bins of bin_len positions counted from each
        range's start (0: one record per range) -> (levels uint8 [rows, 32], row_offsets int64 [n + 1], status int32 [n]),
        torch tensors on the device (event_levels_view reads the records).  Packed (default): range w's records are
        levels[row_offsets[w]:row_offsets[w + 1]]; `capacity` records when given (ranges without room are ERR_BAD_ARG and
        row_offsets[-1] says what all need), otherwise one synchronising sum on the host.  padded_to: row w begins at
        w * padded_to.  The tensors events() returns go in as they are.  The call waits for its result.
        signal: "samples", or "diff" -- the stream's first difference (as in levels()) cut to the ranges: the difference at
        a range's first position is counted, its earlier sample lies in front of the range (x3_signal_range_levels_dev).
        A Fir raises on this keyword: fir_range_levels takes it"""
        sig = level_signal(signal, fir=False)
        return _range_levels_torch(self.ctx, lambda e, *a: self.range_levels_into(*a, signal=sig), "x3_signal_range_levels_dev",
                                   starts, lens, bin_len, padded_to, capacity)

    def fir_range_levels_into(self, d_starts, d_lens, n, bin_len, row_stride, d_levels, rows_cap, d_row_offsets, d_status, fir):
        """range_levels_into on the stream's FIR signal (fir: a Fir or a LevelFir; x3_fir_range_levels_dev); -> rc;
        Context.range_levels_result waits"""
        return self.ctx.fir_range_levels_dev(self.d_x3, self.x3_len, self.d_frame_offsets, self.d_sample_offsets, self.n_frames,
                                             self.params, d_starts, d_lens, n, bin_len, row_stride, d_levels, rows_cap,
                                             d_row_offsets, d_status, self.d_seg_index, self.seg_blocks, fir)

    def fir_range_levels(self, starts, lens, bin_len, fir, *, padded_to=None, capacity=None):
        """range_levels of the stream's FIR signal (levels(signal=fir)) cut to the ranges: the call cuts the filtered stream,
        it does not filter the cut, so a range's first len(taps) - 1 positions are counted, their earlier samples lie in
        front of the range (x3_fir_range_levels_dev).  fir: a Fir; the tensors events(signal=fir) returns go in as they are"""
        if not isinstance(fir, Fir):
            raise ValueError("fir: a Fir")
        return _range_levels_torch(self.ctx, lambda e, *a: self.fir_range_levels_into(*a, fir), "x3_fir_range_levels_dev",
                                   starts, lens, bin_len, padded_to, capacity)

    def tone_range_levels_into(self, d_starts, d_lens, n, bin_len, row_stride, d_levels, rows_cap, d_row_offsets, d_status, tone):
        """range_levels_into on the stream's tone signal, records x3_tone_level (tone: a Tone or a LevelTone;
        x3_tone_range_levels_dev); -> rc; Context.range_levels_result waits"""
        return self.ctx.tone_range_levels_dev(self.d_x3, self.x3_len, self.d_frame_offsets, self.d_sample_offsets, self.n_frames,
                                              self.params, d_starts, d_lens, n, bin_len, row_stride, d_levels, rows_cap,
                                              d_row_offsets, d_status, self.d_seg_index, self.seg_blocks, tone)

    def tone_range_levels(self, starts, lens, bin_len, tone, *, padded_to=None, capacity=None, band=False):
        """range_levels of the stream's tone signal (tone_levels()) cut to the ranges -> (levels, row_offsets, status) as
        range_levels, the records x3_tone_level (TONE_DTYPE: re, im, min, max, n).  The call cuts the stream's signal, it
        does not restart the oscillator: position i of the stream has the phase (i * step) mod 2^32 wherever the range
        begins, so equal samples at different starts give different re and im -- compare band power across ranges, not
        the raw sums.  band=True: x3_tone_power_levels_dev in place behind the call, the records are x3_level records of the
        band's level (LEVEL_DTYPE) and go into events and quantiles; those of ranges without room are the identity.
        tone: a Tone; the tensors events(signal=tone) returns go in as they are (x3_tone_range_levels_dev)"""
        if not isinstance(tone, Tone):
            raise ValueError("tone: a Tone")
        return _range_levels_torch(self.ctx, lambda e, *a: self.tone_range_levels_into(*a, tone), "x3_tone_range_levels_dev",
                                   starts, lens, bin_len, padded_to, capacity, band=band)

    def tone_bank_range_levels_into(self, d_starts, d_lens, n, bin_len, row_stride, d_levels, rows_cap, d_row_offsets, d_status,
                                    tones):
        """tone_range_levels_into for a bank (tones: 1 .. TONE_BANK_MAX Tone or a LevelToneBank): d_levels holds that many
        planes of rows_cap records, plane t at d_levels + 32 * t * rows_cap what tone_range_levels_into writes for tones[t];
        offsets and statuses exist once (x3_tone_bank_range_levels_dev); -> rc; Context.range_levels_result waits"""
        return self.ctx.tone_bank_range_levels_dev(self.d_x3, self.x3_len, self.d_frame_offsets, self.d_sample_offsets,
                                                   self.n_frames, self.params, d_starts, d_lens, n, bin_len, row_stride, d_levels,
                                                   rows_cap, d_row_offsets, d_status, self.d_seg_index, self.seg_blocks, tones)

    def tone_bank_range_levels(self, starts, lens, bin_len, tones, *, padded_to=None, capacity=None, band=False):
        """tone_range_levels for K = len(tones) oscillators (1 .. TONE_BANK_MAX Tone, as tone_bank_levels takes them) from one
        decode of the covering frames -> (levels uint8 [K, rows, 32], row_offsets, status): levels[t] is
        tone_range_levels(starts, lens, bin_len, tones[t], ...)'s records, row_offsets and status are the single call's and
        hold in every plane.  The oscillators are not restarted at a range.  band=True: x3_tone_power_levels_dev in place
        over all planes behind the call, the records are x3_level records of each band's level; those of ranges without
        room are the identity.  The tensors events() returns for any plane go in as they are
        (x3_tone_bank_range_levels_dev)"""
        tones = tone_bank(tones)
        return _range_levels_torch(self.ctx, lambda e, *a: self.tone_bank_range_levels_into(*a, tones),
                                   "x3_tone_bank_range_levels_dev", starts, lens, bin_len, padded_to, capacity, band=band,
                                   planes=len(tones))

    def levels_into(self, bin_len, d_levels, n_bins, d_frame_status=None, signal=LEVEL_SIGNAL_SAMPLES):
        """enqueue x3_signal_levels_dev over this source (device pointers; signal: a LEVEL_SIGNAL_* value), or
        x3_fir_levels_dev (signal: a Fir), or x3_tone_levels_dev and the adapter in place behind it (signal: a Tone); -> rc;
        Context.levels_result waits"""
        if isinstance(signal, Tone):
            return (self.tone_levels_into(bin_len, signal, d_levels, n_bins, d_frame_status)
                    or self.ctx.tone_power_levels_dev(d_levels, n_bins, d_levels))
        call = self.ctx.fir_levels_dev if isinstance(signal, Fir) else self.ctx.signal_levels_dev
        return self._levels_call(call, bin_len, d_levels, n_bins, d_frame_status, signal)

    def _levels_call(self, call, bin_len, d_levels, n_bins, d_frame_status, signal):
        """call: the Context's signal_levels_dev, fir_levels_dev, tone_levels_dev or tone_bank_levels_dev, over this source"""
        return call(self.d_x3, self.x3_len, self.d_frame_offsets, self.d_sample_offsets, self.n_frames, self.params, bin_len,
                    d_levels, n_bins, d_frame_status, self.d_seg_index, self.seg_blocks, signal)

    def _levels_rows(self, bin_len):
        """-> (the bins that cover the stream, no row_first)"""
        return (max(1, -(-self.total // bin_len)) if bin_len else 1), None

    def tone_levels_into(self, bin_len, tone, d_levels, n_bins, d_frame_status=None):
        """enqueue x3_tone_levels_dev over this source (device pointers; tone: a Tone or a LevelTone); -> rc;
        Context.levels_result waits"""
        return self._levels_call(self.ctx.tone_levels_dev, bin_len, d_levels, n_bins, d_frame_status, tone)

    def tone_bank_levels_into(self, bin_len, tones, d_levels, n_bins, d_frame_status=None, *, band=False):
        """enqueue x3_tone_bank_levels_dev over this source (device pointers; tones: 1 .. TONE_BANK_MAX Tone or a
        LevelToneBank; d_levels: that many planes of n_bins records), band=True: and the adapter in place over all planes
        behind it; -> rc; Context.levels_result waits"""
        k = _bank_planes(tones)
        rc = self._levels_call(self.ctx.tone_bank_levels_dev, bin_len, d_levels, n_bins, d_frame_status, tones)
        return rc or (self.ctx.tone_power_levels_dev(d_levels, k * n_bins, d_levels) if band else 0)

    def tone_bank_levels(self, bin_len, tones, n_bins=None, *, band=False):
        """-> (records np.ndarray of TONE_DTYPE [K, n_bins], frame statuses np.int32 [n_frames]): plane t is
        tone_levels(bin_len, tones[t], n_bins), all K = len(tones) of them (1 .. TONE_BANK_MAX Tone) from one pass over
        the stream (x3_tone_bank_levels_dev).  band=True: x3_tone_power_levels_dev in place over all planes behind the
        call; the records are then LEVEL_DTYPE, the level of each band, which events() takes plane by plane"""
        tones = tone_bank(tones)
        return _levels_np(self, "x3_tone_bank_levels_dev", bin_len, n_bins, LEVEL_DTYPE if band else TONE_DTYPE,
                          lambda d_lv, nb, d_st: self.tone_bank_levels_into(bin_len, tones, d_lv, nb, d_st, band=band),
                          planes=len(tones))

    def tone_levels(self, bin_len, tone, n_bins=None):
        """-> (records np.ndarray of TONE_DTYPE [n_bins], frame statuses np.int32 [n_frames]): re, im -- the sums of sample
        times cos and sin of the oscillator's phase -- and the samples' min, max, n per bin of bin_len positions (0: one bin).
        tone: a Tone (x3_tone_levels_dev with the usual table)"""
        if not isinstance(tone, Tone):
            raise ValueError("tone: a Tone")
        return _levels_np(self, "x3_tone_levels_dev", bin_len, n_bins, TONE_DTYPE,
                          lambda d_lv, nb, d_st: self.tone_levels_into(bin_len, tone, d_lv, nb, d_st))

    def levels(self, bin_len, n_bins=None, *, signal="samples"):
        """-> (records np.ndarray of LEVEL_DTYPE [n_bins], frame statuses np.int32 [n_frames]): min, max, n, sum and sum of
        squares per bin of bin_len positions (0: one bin); n_bins: as many as cover the stream unless given.
        signal: "samples", or "diff" -- the samples' first difference, clamped to 16 bits (x3_signal_levels_dev) -- or a
        Fir: the samples behind an integer FIR filter (x3_fir_levels_dev) -- or a Tone: the level of the band at one
        oscillator (x3_tone_levels_dev, then x3_tone_power_levels_dev in place)"""
        sig = level_signal(signal)
        return _levels_np(self, "x3_signal_levels_dev", bin_len, n_bins, LEVEL_DTYPE,
                          lambda d_lv, nb, d_st: self.levels_into(bin_len, d_lv, nb, d_st, sig))

    def events_into(self, d_levels, n_bins, bin_len, rule, d_starts, d_lens, d_event_levels, cap, d_count):
        """enqueue x3_events_dev over n_bins records this source's levels_dev wrote (device pointers; the sample count is the
        last word of the source's sample offsets); -> rc; Context.events_result waits"""
        return self.ctx.events_dev(d_levels, n_bins, bin_len, self.d_sample_offsets + 8 * self.n_frames, rule, d_starts, d_lens,
                                   d_event_levels, cap, d_count)

    def level_quantiles_into(self, d_levels, n_bins, bin_len, key, q_ppm, d_values, d_counted):
        """enqueue x3_level_quantiles_dev over n_bins records this source's levels_dev wrote (device pointers); -> rc;
        Context.level_quantiles_result waits"""
        return self.ctx.level_quantiles_dev(d_levels, n_bins, bin_len, self.d_sample_offsets + 8 * self.n_frames, key, q_ppm,
                                            d_values, d_counted)

    def level_thresholds_into(self, d_levels, n_bins, bin_len, threshold_rule, d_thr):
        """enqueue x3_level_thresholds_dev (one record at d_thr); -> rc; Context.level_quantiles_result waits"""
        return self.ctx.level_thresholds_dev(d_levels, n_bins, bin_len, self.d_sample_offsets + 8 * self.n_frames, threshold_rule,
                                             d_thr)

    def adaptive_events_into(self, d_levels, n_bins, bin_len, rule, d_thr, d_starts, d_lens, d_event_levels, cap, d_count):
        """enqueue x3_events_adaptive_dev with the record at d_thr; -> rc; Context.events_result waits"""
        return self.ctx.events_adaptive_dev(d_levels, n_bins, bin_len, self.d_sample_offsets + 8 * self.n_frames, rule, d_thr,
                                            d_starts, d_lens, d_event_levels, cap, d_count)

    def plane_events_into(self, d_levels, plane_stride, n_bins, bin_len, rule, d_thr, d_starts, d_lens, d_event_planes,
                          d_event_levels, cap, d_count):
        """enqueue x3_plane_events_dev over rule.n_planes planes of n_bins records of this source (device pointers; rule: a
        PlaneEventRule; d_thr: None or a record per plane); -> rc; Context.events_result waits"""
        return self.ctx.plane_events_dev(d_levels, plane_stride, n_bins, bin_len, self.d_sample_offsets + 8 * self.n_frames, rule,
                                         d_thr, d_starts, d_lens, d_event_planes, d_event_levels, cap, d_count)

    def close(self):
        for p in self._own:
            self.ctx.free(p)
        self._own = []


def _frames_samples(data, start):
    """samples the frame headers of data[start:] announce, walked header to header (no CRC checks: a size hint)"""
    n, pos, end = 0, start, len(data)
    while pos + 20 <= end and data[pos] == 0x78 and data[pos + 1] == 0x33:
        n += (data[pos + 4] << 8) | data[pos + 5]
        pos += 20 + ((data[pos + 6] << 8) | data[pos + 7])
    return n


def _read_archives(archives):
    """-> (datas, frame-part starts, sample rates, header statuses, {parameter-set key: (params, [indices])}) of .x3a
    archives (bytes-like objects or paths); an archive whose header does not parse has its status and no group"""
    datas = []
    for a in archives:
        if isinstance(a, (str, os.PathLike)):
            with open(a, "rb") as f:
                datas.append(f.read())
        else:
            datas.append(bytes(a))
    n = len(datas)
    if n == 0:
        raise ValueError("no archives")
    rates = np.zeros(n, dtype=np.uint32)
    statuses = np.zeros(n, dtype=np.int32)
    groups, starts = {}, [0] * n
    for i, d in enumerate(datas):
        rc, rate, p, _ch, hsize = archive_header_read(np.frombuffer(d, dtype=np.uint8))
        if rc:
            statuses[i] = rc
            continue
        rates[i] = rate
        starts[i] = 8 + hsize
        key = bytes(p)
        groups.setdefault(key, (p, []))[1].append(i)
    return datas, starts, rates, statuses, groups


def _frame_parts(datas, starts, idx):
    """one buffer of the archives' frame parts (idx), each at an even offset -> (buf with 16 bytes of slack, its length
    without them, offsets, lengths)"""
    offs, lens, blob, pos = [], [], [], 0
    for i in idx:
        part = datas[i][starts[i]:]
        offs.append(pos)
        lens.append(len(part))
        blob.append(part)
        pos += len(part)
        if pos & 1:
            blob.append(b"\0")
            pos += 1
    return np.frombuffer(b"".join(blob) + b"\0" * 16, dtype=np.uint8), pos, offs, lens


def decode_archives(ctx, archives, row_len=None, fmt=WINDOW_I16):
    """Decode many .x3a archives (bytes-like objects or paths) into padded rows with x3_decode_streams_dev.

    Each archive's header is read on the host (x3_archive_header_read); archives are grouped by parameter set and every
    group is one device call over one buffer of frame parts.  row_len=None: the longest archive's sample count by its frame
    headers, rounded up to a multiple of 4.  Returns (rows [n, row_len] int16 / float32, results (STREAM_RESULT_DTYPE,
    per archive: x3_x3a_decode's n_out, frames_ok, status, frame_errors with wav_cap = row_len), sample rates) in the input
    order.  An archive whose header does not parse gets that status, no samples, and is not sent to the device."""
    datas, starts, rates, statuses, groups = _read_archives(archives)
    n = len(datas)
    results = np.zeros(n, dtype=STREAM_RESULT_DTYPE)
    results["status"] = statuses
    if row_len is None:
        row_len = max([_frames_samples(datas[i], starts[i]) for _, idx in groups.values() for i in idx] + [1])
        row_len = (row_len + 3) // 4 * 4
    esz = 4 if fmt == WINDOW_F32 else 2
    rows = np.zeros((n, row_len), dtype=np.float32 if fmt == WINDOW_F32 else np.int16)
    for p, idx in groups.values():
        buf, pos, offs, lens = _frame_parts(datas, starts, idx)
        m = len(idx)
        d_x3 = ctx.alloc(buf.size)
        d_out = ctx.alloc(esz * m * row_len)
        d_res = ctx.alloc(STREAM_RESULT_DTYPE.itemsize * m)
        try:
            ctx.upload(d_x3, buf)
            rc = ctx.decode_streams_dev(d_x3, pos, offs, lens, p, d_out, row_len, fmt, d_res, flags=STREAMS_ARCHIVE_FRAMES)
            if rc:
                raise X3Error(rc, "x3_decode_streams_dev: " + ctx.last_error())
            rc = ctx.decode_streams_result()[0]
            if rc:
                raise X3Error(rc, "x3_decode_streams_result: " + ctx.last_error())
            rows[idx] = ctx.download(d_out, esz * m * row_len, rows.dtype).reshape(m, row_len)
            results[idx] = ctx.download(d_res, STREAM_RESULT_DTYPE.itemsize * m, STREAM_RESULT_DTYPE)
        finally:
            for ptr in (d_x3, d_out, d_res):
                ctx.free(ptr)
    return rows, results, rates


class Corpus(_Detection):
    """Windows of many streams in HBM (x3_corpus_build / x3_corpus_windows_dev): an index built once over the entries of
    one device buffer, windows addressed as (entry, start).

    `stream`: host bytes (uploaded once, owned) or (d_x3, x3_len) of a device buffer the caller keeps alive.  `offsets` /
    `lengths`: the entries, as in Context.decode_streams_dev.  flags: 0 or STREAMS_ARCHIVE_FRAMES.  seg_blocks: the
    segment index (0: none; it is only ever a hint).  index: "decode" = recorded by a decode of the corpus (block length
    20 and the default codes; none elsewhere), "walk" = built by x3_seg_index_build_dev for any parameters
    (CORPUS_INDEX_WALK).  `.entries`: the entry table (CORPUS_ENTRY_DTYPE)."""
    _has_entries = True   # (_Detection: the calls have an `entries` output)

    def __init__(self, ctx, stream, offsets, lengths, params=None, flags=0, seg_blocks=32, index="decode"):
        self.ctx, self.params, self._h, self._own = ctx, params or Params.default(), None, []
        if index not in ("decode", "walk"):
            raise ValueError('index: "decode" or "walk"')
        offs = np.ascontiguousarray(offsets, dtype=np.uint64)
        lens = np.ascontiguousarray(lengths, dtype=np.uint64)
        if offs.ndim != 1 or offs.size != lens.size:
            raise ValueError("offsets and lengths must be 1-D and of one length")
        if offs.size == 0 or offs.size > 0xFFFFFFF0:
            raise ValueError("a corpus holds 1 .. 0xFFFFFFF0 entries")
        if flags & ~(STREAMS_ARCHIVE_FRAMES | CORPUS_INDEX_WALK):
            raise ValueError("unknown flag")
        if seg_blocks < 0 or seg_blocks % 4 or seg_blocks > 3200:
            raise ValueError("seg_blocks: 0, or a multiple of 4 up to 3200")
        if isinstance(stream, tuple):
            self.d_x3, self.x3_len = stream
        else:
            b = np.ascontiguousarray(stream, dtype=np.uint8)
            self.x3_len = b.size
        if np.any(offs > self.x3_len) or np.any(lens > np.uint64(self.x3_len) - np.minimum(offs, self.x3_len)):
            raise ValueError("an entry lies outside the buffer")
        if not isinstance(stream, tuple):
            self.d_x3 = ctx.alloc(max(b.size, 4))
            self._own.append(self.d_x3)
            ctx.upload(self.d_x3, b)
        h = C.c_void_p(0)
        if index == "walk":
            flags |= CORPUS_INDEX_WALK
        rc = lib().x3_corpus_build(ctx._h, self.d_x3, self.x3_len, offs.ctypes.data, lens.ctypes.data, offs.size, flags,
                                   C.byref(self.params), seg_blocks, C.byref(h))
        if rc:
            self.close()
            raise X3Error(rc, "x3_corpus_build: " + ctx.last_error())
        self._h = h
        ne, nf, tot, sb = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0), C.c_uint32(0)
        lib().x3_corpus_info(h, C.byref(ne), C.byref(nf), C.byref(tot), C.byref(sb))
        self.n_entries, self.n_frames, self.total_samples, self.seg_blocks = ne.value, nf.value, tot.value, sb.value
        self.entries = np.zeros(self.n_entries, dtype=CORPUS_ENTRY_DTYPE)
        lib().x3_corpus_entries(h, self.entries.ctypes.data)
        d_idx, nw = C.c_void_p(0), C.c_uint64(0)
        lib().x3_corpus_seg_index(h, C.byref(d_idx), C.byref(nw))
        d_ent = C.c_void_p(0)
        lib().x3_corpus_entries_dev(h, C.byref(d_ent))
        self.d_entries = d_ent.value   # (the device copy of the entry table; the corpus owns it)
        self.d_seg_index, self.seg_index_words = d_idx.value, nw.value   # (device memory the corpus owns; None, 0: no index)

    @classmethod
    def from_archives(cls, ctx, archives, seg_blocks=32, index="decode"):
        """A corpus of the frame parts of .x3a archives (bytes-like objects or paths), one entry per archive in the input
        order, buffer built as decode_archives builds it.  ValueError for archives of more than one parameter set or with
        a header that does not parse.  `.rates`: the archives' sample rates."""
        datas, starts, rates, statuses, groups = _read_archives(archives)
        if np.any(statuses):
            raise ValueError("archive %d: its header does not parse (status %d)" % (int(np.argmax(statuses != 0)),
                                                                                 int(statuses[statuses != 0][0])))
        if len(groups) != 1:
            raise ValueError("the archives have %d parameter sets; a corpus takes one" % len(groups))
        p, idx = next(iter(groups.values()))
        buf, pos, offs, lens = _frame_parts(datas, starts, idx)
        d_x3 = ctx.alloc(buf.size)
        try:
            ctx.upload(d_x3, buf)
            self = cls(ctx, (d_x3, pos), offs, lens, params=p, flags=STREAMS_ARCHIVE_FRAMES, seg_blocks=seg_blocks,
                       index=index)
        except BaseException:
            ctx.free(d_x3)
            raise
        self._own.append(d_x3)
        self.rates = rates
        return self

    def decode_into(self, d_entries, d_starts, n, length, d_out, fmt, d_status):
        """enqueue n windows (device pointers: d_entries n x u32, d_starts n x u64, d_out n x length, d_status n x i32) ->
        rc; x3_decode_windows_result waits"""
        if self._h is None:
            raise ValueError("the corpus is closed")
        return lib().x3_corpus_windows_dev(self.ctx._h, self._h, d_entries, d_starts, n, length, d_out, fmt, d_status)

    def decode(self, entries, starts, length, fmt=WINDOW_I16):
        """-> (rows np.int16 / np.float32 [n, length], statuses np.int32 [n])"""
        entries = np.ascontiguousarray(entries, dtype=np.uint32)
        starts = np.ascontiguousarray(starts, dtype=np.uint64)
        if entries.shape != starts.shape or entries.ndim != 1 or entries.size == 0:
            raise ValueError("entries and starts: 1-D, non-empty, of one length")
        if length <= 0 or length > 0xFFFFFFFF:
            raise ValueError("length: 1 .. 2^32 - 1")
        n = starts.size
        esz = 4 if fmt == WINDOW_F32 else 2
        d_ent, d_starts, d_out, d_st = (self.ctx.alloc(4 * n), self.ctx.alloc(8 * n), self.ctx.alloc(esz * n * length),
                                        self.ctx.alloc(4 * n))
        try:
            self.ctx.upload(d_ent, entries)
            self.ctx.upload(d_starts, starts)
            rc = self.decode_into(d_ent, d_starts, n, length, d_out, fmt, d_st)
            if rc:
                raise X3Error(rc, "x3_corpus_windows_dev: " + self.ctx.last_error())
            rc = self.ctx.decode_windows_result()[0]
            if rc:
                raise X3Error(rc, "x3_decode_windows_result: " + self.ctx.last_error())
            rows = self.ctx.download(d_out, esz * n * length, np.float32 if fmt == WINDOW_F32 else np.int16)
            return rows.reshape(n, length), self.ctx.download(d_st, 4 * n, np.int32)
        finally:
            for ptr in (d_ent, d_starts, d_out, d_st):
                self.ctx.free(ptr)

    def ranges_into(self, d_entries, d_starts, d_lens, n, row_stride, d_out, out_cap, fmt, d_out_offsets, d_status):
        """enqueue n ranges (device pointers: d_entries n x u32, d_starts n x u64, d_lens n x u32, d_out out_cap samples,
        d_out_offsets (n + 1) x u64 or None when padded, d_status n x i32); row_stride 0: packed; -> rc;
        Context.decode_ranges_result waits"""
        if self._h is None:
            raise ValueError("the corpus is closed")
        return lib().x3_corpus_ranges_dev(self.ctx._h, self._h, d_entries, d_starts, d_lens, n, row_stride, d_out, out_cap,
                                          fmt, d_out_offsets, d_status)

    def ranges(self, entries, starts, lens, *, padded_to=None, capacity=None, dtype=None):
        """Variable-length windows [starts[w], starts[w] + lens[w]) of entry entries[w] -> (out, offsets, status), torch
        tensors on the device; layout, capacity (default: one synchronising sum of the lengths), padded_to and dtype as
        WindowSource.ranges."""
        import torch
        return _ranges_torch(self.ctx, self.ranges_into, "x3_corpus_ranges_dev", starts, lens, padded_to, capacity,
                             dtype or torch.int16, entries=entries)

    def range_spectra_into(self, d_entries, d_starts, d_lens, n, rule, d_samples, samples_cap, d_sample_offsets, row_stride,
                           d_out, rows_cap, d_row_offsets, d_status):
        """WindowSource.range_spectra_into on ranges of entries (d_entries n x u32)"""
        return _range_spectra_enqueue(self.ctx, self.ranges_into)(
            d_entries, d_starts, d_lens, n, rule, d_samples, samples_cap, d_sample_offsets, row_stride, d_out, rows_cap,
            d_row_offsets, d_status)

    def range_spectra(self, entries, starts, lens, n_fft, hop=None, *, power=True, table=None, padded_to=None, capacity=None,
                      sample_capacity=None):
        """WindowSource.range_spectra on the ranges [starts[w], starts[w] + lens[w]) of entry entries[w]"""
        return _range_spectra_torch(self.ctx, _range_spectra_enqueue(self.ctx, self.ranges_into), "x3_corpus_ranges_dev", starts,
                                    lens, n_fft, hop, power, table, padded_to, capacity, sample_capacity, entries=entries)

    def range_band_levels_into(self, d_entries, d_starts, d_lens, n, rule, fold, d_samples, samples_cap, d_sample_offsets,
                               row_stride, d_levels, rows_cap, d_row_offsets, d_status):
        """WindowSource.range_band_levels_into on ranges of entries (d_entries n x u32)"""
        return _range_spectra_enqueue(self.ctx, self.ranges_into)(
            d_entries, d_starts, d_lens, n, rule, d_samples, samples_cap, d_sample_offsets, row_stride, d_levels, rows_cap,
            d_row_offsets, d_status, fold=fold)

    def range_band_levels(self, entries, starts, lens, n_fft, hop=None, *, frames_per_bin=1, bands=None, table=None,
                          padded_to=None, capacity=None, sample_capacity=None):
        """WindowSource.range_band_levels on the ranges [starts[w], starts[w] + lens[w]) of entry entries[w]"""
        return _range_spectra_torch(self.ctx, _range_spectra_enqueue(self.ctx, self.ranges_into), "x3_corpus_ranges_dev", starts,
                                    lens, n_fft, hop, True, table, padded_to, capacity, sample_capacity, entries=entries,
                                    fold=_BandFold(frames_per_bin, bands))

    def range_levels_into(self, d_entries, d_starts, d_lens, n, bin_len, row_stride, d_levels, rows_cap, d_row_offsets, d_status,
                          signal=LEVEL_SIGNAL_SAMPLES):
        """enqueue the level records of n ranges of entries (device pointers: d_entries n x u32, the rest as
        WindowSource.range_levels_into); -> rc; Context.range_levels_result waits"""
        if self._h is None:
            raise ValueError("the corpus is closed")
        if isinstance(signal, (Fir, Tone)):
            level_signal(signal, fir=False)   # (raises: "not built yet" on this keyword; fir_range_levels_into takes a Fir)
        return self.ctx.corpus_signal_range_levels_dev(self, d_entries, d_starts, d_lens, n, bin_len, row_stride, d_levels,
                                                       rows_cap, d_row_offsets, d_status, signal)

    def range_levels(self, entries, starts, lens, bin_len, *, padded_to=None, capacity=None, signal="samples"):
        """The x3_level records of the ranges [starts[w], starts[w] + lens[w]) of entry entries[w] -> (levels, row_offsets,
        status) as WindowSource.range_levels; the tensors events() returns go in as they are.  signal: as there -- the
        entry's first difference cut to the ranges; no difference crosses from one entry into the next.  A Fir raises on
        this keyword: fir_range_levels takes it"""
        sig = level_signal(signal, fir=False)
        return _range_levels_torch(self.ctx, lambda *a: self.range_levels_into(*a, signal=sig),
                                   "x3_corpus_signal_range_levels_dev", starts, lens, bin_len, padded_to, capacity, entries=entries)

    def fir_range_levels_into(self, d_entries, d_starts, d_lens, n, bin_len, row_stride, d_levels, rows_cap, d_row_offsets,
                              d_status, fir):
        """range_levels_into on each entry's FIR signal (fir: a Fir or a LevelFir; x3_corpus_fir_range_levels_dev); -> rc"""
        if self._h is None:
            raise ValueError("the corpus is closed")
        return self.ctx.corpus_fir_range_levels_dev(self, d_entries, d_starts, d_lens, n, bin_len, row_stride, d_levels, rows_cap,
                                                    d_row_offsets, d_status, fir)

    def fir_range_levels(self, entries, starts, lens, bin_len, fir, *, padded_to=None, capacity=None):
        """WindowSource.fir_range_levels for ranges of entries; no filter history crosses from one entry into the next"""
        if not isinstance(fir, Fir):
            raise ValueError("fir: a Fir")
        return _range_levels_torch(self.ctx, lambda *a: self.fir_range_levels_into(*a, fir), "x3_corpus_fir_range_levels_dev",
                                   starts, lens, bin_len, padded_to, capacity, entries=entries)

    def tone_range_levels_into(self, d_entries, d_starts, d_lens, n, bin_len, row_stride, d_levels, rows_cap, d_row_offsets,
                               d_status, tone):
        """range_levels_into on each entry's tone signal, records x3_tone_level (tone: a Tone or a LevelTone;
        x3_corpus_tone_range_levels_dev); -> rc"""
        if self._h is None:
            raise ValueError("the corpus is closed")
        return self.ctx.corpus_tone_range_levels_dev(self, d_entries, d_starts, d_lens, n, bin_len, row_stride, d_levels,
                                                     rows_cap, d_row_offsets, d_status, tone)

    def tone_range_levels(self, entries, starts, lens, bin_len, tone, *, padded_to=None, capacity=None, band=False):
        """WindowSource.tone_range_levels for ranges of entries; the phase is 0 at every entry's first position"""
        if not isinstance(tone, Tone):
            raise ValueError("tone: a Tone")
        return _range_levels_torch(self.ctx, lambda *a: self.tone_range_levels_into(*a, tone), "x3_corpus_tone_range_levels_dev",
                                   starts, lens, bin_len, padded_to, capacity, entries=entries, band=band)

    def tone_bank_range_levels_into(self, d_entries, d_starts, d_lens, n, bin_len, row_stride, d_levels, rows_cap, d_row_offsets,
                                    d_status, tones):
        """tone_range_levels_into for a bank (tones: 1 .. TONE_BANK_MAX Tone or a LevelToneBank): that many planes of
        rows_cap records in d_levels (x3_corpus_tone_bank_range_levels_dev); -> rc"""
        if self._h is None:
            raise ValueError("the corpus is closed")
        return self.ctx.corpus_tone_bank_range_levels_dev(self, d_entries, d_starts, d_lens, n, bin_len, row_stride, d_levels,
                                                          rows_cap, d_row_offsets, d_status, tones)

    def tone_bank_range_levels(self, entries, starts, lens, bin_len, tones, *, padded_to=None, capacity=None, band=False):
        """WindowSource.tone_bank_range_levels for ranges of entries; the phase is 0 at every entry's first position in every
        plane"""
        tones = tone_bank(tones)
        return _range_levels_torch(self.ctx, lambda *a: self.tone_bank_range_levels_into(*a, tones),
                                   "x3_corpus_tone_bank_range_levels_dev", starts, lens, bin_len, padded_to, capacity,
                                   entries=entries, band=band, planes=len(tones))

    def levels_rows(self, bin_len):
        """-> row_first np.uint64 [n_entries + 1]: entry e's rows of levels() are [row_first[e], row_first[e + 1])"""
        if self._h is None:
            raise ValueError("the corpus is closed")
        rf = np.zeros(self.entries.size + 1, dtype=np.uint64)
        rc = lib().x3_corpus_levels_rows(self._h, bin_len, rf.ctypes.data)
        if rc:
            raise X3Error(rc, "x3_corpus_levels_rows")
        return rf

    def levels_into(self, bin_len, d_levels, n_rows, d_frame_status=None, signal=LEVEL_SIGNAL_SAMPLES):
        """enqueue x3_corpus_signal_levels_dev (device pointers; signal: a LEVEL_SIGNAL_* value), or
        x3_corpus_fir_levels_dev (signal: a Fir), or x3_corpus_tone_levels_dev and the adapter in place behind it (signal: a
        Tone); -> rc; Context.levels_result waits"""
        if self._h is None:
            raise ValueError("the corpus is closed")
        if isinstance(signal, Tone):
            return (self.tone_levels_into(bin_len, signal, d_levels, n_rows, d_frame_status)
                    or self.ctx.tone_power_levels_dev(d_levels, n_rows, d_levels))
        call = self.ctx.corpus_fir_levels_dev if isinstance(signal, Fir) else self.ctx.corpus_signal_levels_dev
        return call(self, bin_len, d_levels, n_rows, d_frame_status, signal)

    def _levels_rows(self, bin_len):
        """-> (the rows of all entries, row_first)"""
        rf = self.levels_rows(bin_len)
        return int(rf[-1]), rf

    def levels(self, bin_len, *, signal="samples"):
        """-> (records np.ndarray of LEVEL_DTYPE [rows], row_first np.uint64 [n_entries + 1], frame statuses np.int32
        [n_frames]): the levels of every entry, positions relative to the entry, bins of bin_len positions (0: one bin).
        signal: "samples";
        "diff" -- the samples' first difference, clamped to 16 bits (x3_corpus_signal_levels_dev);
        a Fir -- the samples behind an integer FIR filter (x3_corpus_fir_levels_dev);
        a Tone -- the level of the band at one oscillator (x3_corpus_tone_levels_dev, then x3_tone_power_levels_dev in
        place).
        Every entry stands alone: no difference and no filter history crosses from one entry into the next, and a Tone's
        phase is 0 at every entry's start"""
        sig = level_signal(signal)
        return _levels_np(self, "x3_corpus_signal_levels_dev", bin_len, None, LEVEL_DTYPE,
                          lambda d_lv, n_rows, d_st: self.levels_into(bin_len, d_lv, n_rows, d_st, sig))

    def tone_levels_into(self, bin_len, tone, d_levels, n_rows, d_frame_status=None):
        """enqueue x3_corpus_tone_levels_dev (device pointers; tone: a Tone or a LevelTone); -> rc; Context.levels_result
        waits"""
        if self._h is None:
            raise ValueError("the corpus is closed")
        return self.ctx.corpus_tone_levels_dev(self, bin_len, d_levels, n_rows, d_frame_status, tone)

    def tone_bank_levels_into(self, bin_len, tones, d_levels, n_rows, d_frame_status=None, *, band=False):
        """enqueue x3_corpus_tone_bank_levels_dev (device pointers; tones: 1 .. TONE_BANK_MAX Tone or a LevelToneBank;
        d_levels: that many planes of n_rows records), band=True: and the adapter in place over all planes behind it; -> rc;
        Context.levels_result waits"""
        if self._h is None:
            raise ValueError("the corpus is closed")
        k = _bank_planes(tones)
        rc = self.ctx.corpus_tone_bank_levels_dev(self, bin_len, d_levels, n_rows, d_frame_status, tones)
        return rc or (self.ctx.tone_power_levels_dev(d_levels, k * n_rows, d_levels) if band else 0)

    def tone_bank_levels(self, bin_len, tones, *, band=False):
        """-> (records np.ndarray of TONE_DTYPE [K, rows], row_first, frame statuses): plane t is tone_levels(bin_len,
        tones[t])'s records, all K = len(tones) of them (1 .. TONE_BANK_MAX Tone) from one pass over the corpus
        (x3_corpus_tone_bank_levels_dev); row_first is the single call's, in every plane.  band=True: the adapter in place
        over all planes, the records are LEVEL_DTYPE"""
        tones = tone_bank(tones)
        return _levels_np(self, "x3_corpus_tone_bank_levels_dev", bin_len, None, LEVEL_DTYPE if band else TONE_DTYPE,
                          lambda d_lv, n_rows, d_st: self.tone_bank_levels_into(bin_len, tones, d_lv, n_rows, d_st, band=band),
                          planes=len(tones))

    def tone_levels(self, bin_len, tone):
        """-> (records np.ndarray of TONE_DTYPE [rows], row_first, frame statuses) as levels(): the quadrature sums of every
        entry's bins against one oscillator, whose phase restarts at 0 with every entry (x3_corpus_tone_levels_dev)"""
        if not isinstance(tone, Tone):
            raise ValueError("tone: a Tone")
        return _levels_np(self, "x3_corpus_tone_levels_dev", bin_len, None, TONE_DTYPE,
                          lambda d_lv, n_rows, d_st: self.tone_levels_into(bin_len, tone, d_lv, n_rows, d_st))

    def events_into(self, d_levels, n_rows, bin_len, rule, d_entries, d_starts, d_lens, d_event_levels, cap, d_count):
        """enqueue x3_corpus_events_dev over the n_rows records Context.corpus_levels_dev wrote (device pointers); -> rc;
        Context.events_result waits"""
        if self._h is None:
            raise ValueError("the corpus is closed")
        return self.ctx.corpus_events_dev(self, d_levels, n_rows, bin_len, rule, d_entries, d_starts, d_lens, d_event_levels,
                                          cap, d_count)

    def level_quantiles_into(self, d_levels, n_rows, bin_len, key, q_ppm, d_values, d_counted):
        """enqueue x3_corpus_level_quantiles_dev over the n_rows records Context.corpus_levels_dev wrote; -> rc;
        Context.level_quantiles_result waits"""
        if self._h is None:
            raise ValueError("the corpus is closed")
        return self.ctx.corpus_level_quantiles_dev(self, d_levels, n_rows, bin_len, key, q_ppm, d_values, d_counted)

    def level_thresholds_into(self, d_levels, n_rows, bin_len, threshold_rule, d_thr):
        """enqueue x3_corpus_level_thresholds_dev (n_entries records at d_thr); -> rc"""
        if self._h is None:
            raise ValueError("the corpus is closed")
        return self.ctx.corpus_level_thresholds_dev(self, d_levels, n_rows, bin_len, threshold_rule, d_thr)

    def adaptive_events_into(self, d_levels, n_rows, bin_len, rule, d_thr, d_entries, d_starts, d_lens, d_event_levels, cap,
                             d_count):
        """enqueue x3_corpus_events_adaptive_dev with entry e's thresholds at d_thr[e]; -> rc; Context.events_result waits"""
        if self._h is None:
            raise ValueError("the corpus is closed")
        return self.ctx.corpus_events_adaptive_dev(self, d_levels, n_rows, bin_len, rule, d_thr, d_entries, d_starts, d_lens,
                                                   d_event_levels, cap, d_count)

    def plane_events_into(self, d_levels, plane_stride, n_rows, bin_len, rule, d_thr, d_entries, d_starts, d_lens, d_event_planes,
                          d_event_levels, cap, d_count):
        """enqueue x3_corpus_plane_events_dev over rule.n_planes planes of the n_rows records Context.corpus_levels_dev wrote
        (device pointers; d_thr: None or records [n_planes, n_entries]); -> rc; Context.events_result waits"""
        if self._h is None:
            raise ValueError("the corpus is closed")
        return self.ctx.corpus_plane_events_dev(self, d_levels, plane_stride, n_rows, bin_len, rule, d_thr, d_entries, d_starts,
                                                d_lens, d_event_planes, d_event_levels, cap, d_count)

    def close(self):
        if self._h is not None:
            lib().x3_corpus_destroy(self._h)
            self._h = None
        for ptr in self._own:
            self.ctx.free(ptr)
        self._own = []
