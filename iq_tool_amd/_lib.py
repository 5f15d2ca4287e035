"""ctypes loader for libiqgpu.so.  Fails loudly when the HIP library is missing: there is no
CPU fallback anywhere in this package."""
import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("IQGPU_LIB") or os.path.join(HERE, "lib", "libiqgpu.so")

FMT = dict(cu8=8, cs8=9, cu16=10, cs16=11, cs24=12, cu32=13, cs32=14, cf32=15, sc16q11=16)
FMT_NAME = {v: k for k, v in FMT.items()}
BYTES_PER_FRAME = {8: 2, 9: 2, 10: 4, 11: 4, 16: 4, 12: 6, 13: 8, 14: 8, 15: 8}
FILTER = dict(none=0, lowpass=1, highpass=2, passband=3, stopband=4)
FILTER_IMPL = dict(auto=0, fir=1, fft=2)
K_NAMES = ("dc_prefix", "dc_scan", "front", "filter", "move", "agc", "cascade")

ERRORS = {0: "OK", -1: "EINVAL", -2: "ENODEV", -3: "ENOMEM", -4: "ERATIO", -5: "EFORMAT", -6: "ESHIFT",
          -7: "EFILTER", -8: "ECAPACITY", -9: "EHIP", -10: "EUNSUPPORTED"}


class FilterReq(C.Structure):
    _fields_ = [("type", C.c_int), ("f1_hz", C.c_float), ("f2_hz", C.c_float)]


class ChainDesc(C.Structure):
    _fields_ = [("in_format", C.c_int), ("out_format", C.c_int),
                ("input_rate_hz", C.c_double), ("target_rate_hz", C.c_double),
                ("resample_ratio", C.c_float), ("gain", C.c_float),
                ("shift_hz", C.c_double), ("shift_after_resample", C.c_int),
                ("dc_block_enable", C.c_int),
                ("iq_correct_enable", C.c_int), ("iq_mag", C.c_float), ("iq_phase", C.c_float),
                ("no_resample", C.c_int),
                ("n_filters", C.c_int), ("filters", FilterReq * 5),
                ("transition_width_hz", C.c_float), ("attenuation_db", C.c_float),
                ("filter_taps", C.c_int), ("filter_impl", C.c_int), ("fft_size", C.c_int),
                ("device_ordinal", C.c_int), ("block_samples", C.c_size_t),
                ("agc_enable", C.c_int), ("agc_profile", C.c_int), ("agc_target", C.c_float),
                ("agc_clock", C.c_int), ("agc_chunk_frames", C.c_uint32)]


class AgcState(C.Structure):
    _fields_ = [("locked", C.c_int), ("peak_memory", C.c_float), ("current_gain", C.c_float),
                ("reserved", C.c_int), ("last_strong_peak_time", C.c_double), ("samples_seen", C.c_uint64)]


class AgcChunk(C.Structure):
    """iqgpu_agc_chunk: one row of iqgpu_chain_measure's table"""
    _fields_ = [("peak2", C.c_double), ("frames_out", C.c_uint32), ("reserved", C.c_uint32)]


class DcState(C.Structure):
    """iqgpu_dc_state: the DC blocker's state, in double as the chain keeps it"""
    _fields_ = [("re", C.c_double), ("im", C.c_double)]


class DcRow(C.Structure):
    """iqgpu_dc_row: the map of one call, v_after = f * v_before + g"""
    _fields_ = [("f", C.c_double), ("g_re", C.c_double), ("g_im", C.c_double), ("frames", C.c_uint64)]


class StateInfo(C.Structure):
    """iqgpu_state_info: the header figures of a saved chain state (iqgpu_state_inspect)"""
    _fields_ = [("format_version", C.c_uint32), ("reserved", C.c_uint32), ("bytes", C.c_uint64), ("fingerprint", C.c_uint64),
                ("frames_in", C.c_uint64), ("frames_out", C.c_uint64)]


class ChainInfo(C.Structure):
    _fields_ = [("ratio", C.c_float), ("interp", C.c_int), ("num_halfband_stages", C.c_int),
                ("stage_m", C.c_int * 16), ("rate_arb", C.c_float), ("arb_step", C.c_uint32),
                ("nco_dtheta", C.c_uint32), ("dc_alpha", C.c_float),
                ("filter_post_resample", C.c_int), ("filter_impl", C.c_int),
                ("filter_ntaps", C.c_uint32), ("filter_block", C.c_uint32),
                ("history_samples", C.c_uint32)]


class Profile(C.Structure):
    _fields_ = [("launches", C.c_uint64 * 8), ("ms", C.c_double * 8)]


class IqOptimizerStats(C.Structure):
    _fields_ = [("calls", C.c_uint64), ("runs", C.c_uint64), ("skipped_interval", C.c_uint64),
                ("skipped_power", C.c_uint64), ("accepted", C.c_uint64),
                ("initial_metric", C.c_float), ("final_metric", C.c_float),
                ("average_power_db", C.c_float), ("power_range_db", C.c_float)]


RAND_DIR_FN = C.CFUNCTYPE(C.c_float, C.c_void_p)


class IqCand(C.Structure):
    """iqgpu_iq_cand: one candidate pair of correction factors"""
    _fields_ = [("mag", C.c_float), ("phase", C.c_float)]


class IqCalibOpts(C.Structure):
    """iqgpu_iq_calib_opts: the options of the calibration search (iqgpu_iq_calib_opts_init sets the defaults)"""
    _fields_ = [("max_blocks", C.c_uint32), ("grid", C.c_uint32), ("span", C.c_float), ("min_step", C.c_float),
                ("power_threshold_db", C.c_float), ("center_mag", C.c_float), ("center_phase", C.c_float)]


class IqCalibLevel(C.Structure):
    _fields_ = [("center_mag", C.c_float), ("center_phase", C.c_float), ("step", C.c_float), ("pick", C.c_uint32),
                ("reserved", C.c_uint32), ("total_at_pick", C.c_double)]


class IqCalibReport(C.Structure):
    """iqgpu_iq_calib_report: the result of a calibration with its level trace"""
    _fields_ = [("found", C.c_int), ("mag", C.c_float), ("phase", C.c_float),
                ("total_at_center0", C.c_double), ("total_at_best", C.c_double),
                ("blocks_taken", C.c_uint32), ("blocks_used", C.c_uint32), ("n_levels", C.c_uint32), ("evaluations", C.c_uint32),
                ("level", IqCalibLevel * 16)]


PSD_WINDOW = dict(rect=0, hann=1, hamming=2, blackman_harris=3)


class PsdOpts(C.Structure):
    """iqgpu_psd_opts: the options of a power-spectrum accumulator (iqgpu_psd_opts_init sets the defaults)"""
    _fields_ = [("nfft", C.c_uint32), ("hop", C.c_uint32), ("window", C.c_int), ("gain", C.c_float)]


class PsdInfo(C.Structure):
    """iqgpu_psd_info: what iqgpu_psd_read reports beside the two arrays"""
    _fields_ = [("frames", C.c_uint64), ("segments", C.c_uint64), ("nfft", C.c_uint32), ("hop", C.c_uint32),
                ("window_sum", C.c_double), ("window_sum_sq", C.c_double)]


class SgramOpts(C.Structure):
    """iqgpu_sgram_opts: the options of a row accumulator (iqgpu_sgram_opts_init sets the defaults)"""
    _fields_ = [("nfft", C.c_uint32), ("hop", C.c_uint32), ("window", C.c_int), ("gain", C.c_float), ("row_segments", C.c_uint32)]


class SgramInfo(C.Structure):
    """iqgpu_sgram_info: what iqgpu_sgram_read_open reports beside the two arrays"""
    _fields_ = [("frames", C.c_uint64), ("segments", C.c_uint64), ("rows", C.c_uint64), ("open_segments", C.c_uint32),
                ("nfft", C.c_uint32), ("hop", C.c_uint32), ("row_segments", C.c_uint32),
                ("window_sum", C.c_double), ("window_sum_sq", C.c_double)]


class StatsResult(C.Structure):
    """iqgpu_stats_result: what iqgpu_stats_read reports and iqgpu_stats_merge concatenates"""
    _fields_ = [("frames", C.c_uint64), ("nonfinite_frames", C.c_uint64), ("rail_lo", C.c_uint64 * 2), ("rail_hi", C.c_uint64 * 2),
                ("hist", (C.c_uint64 * 256) * 2), ("min", C.c_float * 2), ("max", C.c_float * 2),
                ("peak_power", C.c_double), ("peak_frame", C.c_uint64),
                ("sum", C.c_double * 2), ("sum_sq", C.c_double * 2), ("sum_iq", C.c_double)]


class StatsDerived(C.Structure):
    """iqgpu_stats_derived: the figures iqgpu_stats_derive computes from a result"""
    _fields_ = [("n", C.c_uint64), ("mean_i", C.c_double), ("mean_q", C.c_double), ("power", C.c_double), ("rms_dbfs", C.c_double),
                ("peak_dbfs", C.c_double), ("crest_db", C.c_double), ("var_i", C.c_double), ("var_q", C.c_double),
                ("iq_gain_ratio", C.c_double), ("iq_phase_rad", C.c_double), ("clip_fraction", C.c_double), ("bins_used", C.c_uint32 * 2)]


class EnvOpts(C.Structure):
    """iqgpu_env_opts: the option of an envelope accumulator (iqgpu_env_opts_init sets the default)"""
    _fields_ = [("block_frames", C.c_uint32)]


class EnvInfo(C.Structure):
    """iqgpu_env_info: what iqgpu_env_read_open reports beside the open row"""
    _fields_ = [("frames", C.c_uint64), ("rows", C.c_uint64), ("nonfinite_frames", C.c_uint64), ("open_frames", C.c_uint32),
                ("block_frames", C.c_uint32)]


class LagOpts(C.Structure):
    """iqgpu_lag_opts: the options of a lag-product accumulator (iqgpu_lag_opts_init sets the defaults)"""
    _fields_ = [("block_frames", C.c_uint32), ("n_lags", C.c_uint32), ("lags", C.c_uint32 * 4)]


class LagInfo(C.Structure):
    """iqgpu_lag_info: what iqgpu_lag_read_open reports beside the open row"""
    _fields_ = [("frames", C.c_uint64), ("rows", C.c_uint64), ("nonfinite_frames", C.c_uint64), ("open_frames", C.c_uint32),
                ("block_frames", C.c_uint32), ("n_lags", C.c_uint32), ("lags", C.c_uint32 * 4)]


class LagEstimate(C.Structure):
    """iqgpu_lag_estimate: what iqgpu_lag_estimate_rows derives from a range of rows"""
    _fields_ = [("re", C.c_double), ("im", C.c_double), ("power", C.c_double), ("hz", C.c_double), ("coherence", C.c_double),
                ("span_hz", C.c_double)]


class MatchOpts(C.Structure):
    """iqgpu_match_opts: the options of a template-correlation accumulator (iqgpu_match_opts_init sets the defaults)"""
    _fields_ = [("nfft", C.c_uint32), ("block_frames", C.c_uint32), ("n_templates", C.c_uint32), ("template_frames", C.c_uint32)]


class MatchInfo(C.Structure):
    """iqgpu_match_info: what iqgpu_match_read_open reports beside the open row"""
    _fields_ = [("frames", C.c_uint64), ("segments", C.c_uint64), ("rows", C.c_uint64), ("open_segments", C.c_uint32),
                ("nfft", C.c_uint32), ("block_frames", C.c_uint32), ("n_templates", C.c_uint32), ("template_frames", C.c_uint32),
                ("reserved", C.c_uint32), ("template_energy", C.c_double * 8)]


class MatchPeak(C.Structure):
    """iqgpu_match_peak: one detection iqgpu_match_peaks found"""
    _fields_ = [("first_frame", C.c_uint64), ("template_index", C.c_uint32), ("peak", C.c_float), ("ratio", C.c_double)]


class EnvBurstOpts(C.Structure):
    """iqgpu_env_burst_opts: the rules of iqgpu_env_bursts"""
    _fields_ = [("block_frames", C.c_uint32), ("min_rows", C.c_uint32), ("hang_rows", C.c_uint32), ("pad_rows", C.c_uint32),
                ("on", C.c_double), ("off", C.c_double)]


class EnvBurst(C.Structure):
    """iqgpu_env_burst: one range iqgpu_env_bursts found"""
    _fields_ = [("first_frame", C.c_uint64), ("frames", C.c_uint64), ("peak_row", C.c_uint64), ("peak_mean", C.c_double)]


class WavInfo(C.Structure):
    _fields_ = [("source_software", C.c_int),
                ("software_name", C.c_char * 64), ("software_version", C.c_char * 64), ("radio_model", C.c_char * 128),
                ("software_name_present", C.c_int), ("software_version_present", C.c_int), ("radio_model_present", C.c_int),
                ("center_freq_hz", C.c_double), ("center_freq_hz_present", C.c_int),
                ("timestamp_unix", C.c_int64), ("timestamp_unix_present", C.c_int),
                ("timestamp_str", C.c_char * 64), ("timestamp_str_present", C.c_int),
                ("sdr_info_present", C.c_int),
                ("sample_rate", C.c_int32), ("channels", C.c_int32), ("bits_per_sample", C.c_int32), ("format_tag", C.c_int32),
                ("in_format", C.c_int),
                ("data_offset", C.c_uint64), ("data_bytes", C.c_uint64), ("frames", C.c_uint64)]


class IqgpuError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("libiqgpu %s (%d): %s" % (ERRORS.get(code, "?"), code, msg))
        self.code = code


# every symbol include/iqgpu.h declares: (name, restype, argtypes)
_vp, _sz = C.c_void_p, C.c_size_t



def _with_device(name, res, args):
    """an entry point that takes host memory and its _device form: the same signature"""
    return (name, res, args), (name + "_device", res, args)


SYMBOLS = [
    ("iqgpu_abi_version", C.c_int, []),
    ("iqgpu_last_error", C.c_char_p, []),
    ("iqgpu_device_count", C.c_int, []),
    ("iqgpu_device_pci_bus_id", C.c_int, [C.c_int, C.c_char_p, _sz]),
    ("iqgpu_device_numa_node", C.c_int, [C.c_int, C.POINTER(C.c_int), C.c_char_p, _sz]),
    ("iqgpu_bind_thread_to_device", C.c_int, [C.c_int, C.POINTER(C.c_int)]),
    ("iqgpu_chain_desc_init", None, [C.POINTER(ChainDesc)]),
    ("iqgpu_chain_create", C.c_int, [C.POINTER(ChainDesc), C.POINTER(_vp)]),
    ("iqgpu_chain_destroy", None, [_vp]),
    ("iqgpu_chain_get_info", C.c_int, [_vp, C.POINTER(ChainInfo)]),
    ("iqgpu_chain_get_filter_taps", C.c_int, [_vp, _vp, _sz]),
    ("iqgpu_design_probe", C.c_int, [C.POINTER(ChainDesc), C.POINTER(ChainInfo), _vp, _sz, _vp, _sz, _vp, _sz]),
    ("iqgpu_design_out_frames", C.c_int, [C.POINTER(ChainDesc), _sz, C.POINTER(_sz)]),
    ("iqgpu_design_preroll_frames", C.c_int, [C.POINTER(ChainDesc), C.POINTER(C.c_uint64)]),
    ("iqgpu_design_out_frames_range", C.c_int, [C.POINTER(ChainDesc), C.c_uint64, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    *_with_device("iqgpu_chain_process", C.c_int, [_vp, _vp, _sz, _vp, _sz, C.POINTER(_sz)]),
    ("iqgpu_chain_submit", C.c_int, [_vp, _vp, _sz, _vp, _sz, C.POINTER(_sz), C.POINTER(C.c_uint64)]),
    ("iqgpu_chain_collect", C.c_int, [_vp, C.c_uint64]),
    ("iqgpu_chain_pipeline_depth", C.c_int, []),
    ("iqgpu_chain_reset", C.c_int, [_vp]),
    *_with_device("iqgpu_chain_seek", C.c_int, [_vp, C.c_uint64, _vp, _sz]),
    *_with_device("iqgpu_chain_measure", C.c_int, [_vp, _vp, _sz, _vp, _sz, C.POINTER(_sz)]),
    ("iqgpu_chain_measure_submit", C.c_int, [_vp, _vp, _sz, _vp, _sz, C.POINTER(_sz), C.POINTER(C.c_uint64)]),
    ("iqgpu_chain_agc_advance", C.c_int, [_vp, C.POINTER(AgcState), _vp, _sz, _vp]),
    ("iqgpu_chain_agc_initial_state", C.c_int, [_vp, C.POINTER(AgcState)]),
    *_with_device("iqgpu_chain_seek_agc", C.c_int, [_vp, C.c_uint64, _vp, _sz, C.POINTER(AgcState)]),
    ("iqgpu_chain_get_agc_state", C.c_int, [_vp, C.POINTER(AgcState)]),
    ("iqgpu_chain_get_dc_state", C.c_int, [_vp, C.POINTER(DcState)]),
    *_with_device("iqgpu_chain_dc_measure", C.c_int, [_vp, C.c_uint64, _vp, _sz, C.POINTER(DcRow)]),
    ("iqgpu_chain_dc_advance", C.c_int, [_vp, C.POINTER(DcState), _vp, _sz, _vp]),
    *_with_device("iqgpu_chain_seek_dc", C.c_int, [_vp, C.c_uint64, _vp, _sz, _sz, C.POINTER(DcState)]),
    *_with_device("iqgpu_chain_dcagc_dc_measure", C.c_int, [_vp, C.c_uint64, _vp, _sz, _vp, _sz, C.POINTER(_sz)]),
    ("iqgpu_chain_dcagc_dc_advance", C.c_int, [_vp, C.POINTER(DcState), _vp, _sz, _vp]),
    *_with_device("iqgpu_chain_dcagc_seek", C.c_int, [_vp, C.c_uint64, _vp, _sz, _sz, C.POINTER(DcState), C.POINTER(AgcState)]),
    *_with_device("iqgpu_chain_dcagc_measure", C.c_int, [_vp, _vp, _sz, _vp, _sz, C.POINTER(_sz)]),
    ("iqgpu_design_preroll_frames_rms", C.c_int, [C.POINTER(ChainDesc), C.POINTER(C.c_uint64)]),
    *_with_device("iqgpu_chain_seek_rms", C.c_int, [_vp, C.c_uint64, _vp, _sz]),
    ("iqgpu_design_preroll_frames_dcrms", C.c_int, [C.POINTER(ChainDesc), C.POINTER(C.c_uint64)]),
    *_with_device("iqgpu_chain_dcrms_dc_measure", C.c_int, [_vp, C.c_uint64, _vp, _sz, C.POINTER(DcRow)]),
    ("iqgpu_chain_dcrms_dc_advance", C.c_int, [_vp, C.POINTER(DcState), _vp, _sz, _vp]),
    *_with_device("iqgpu_chain_dcrms_seek", C.c_int, [_vp, C.c_uint64, _vp, _sz, _sz, C.POINTER(DcState)]),
    *_with_device("iqgpu_chain_dc_measure_range", C.c_int, [_vp, C.c_uint64, _vp, _sz, _sz, _vp, _sz, C.POINTER(_sz), _vp]),
    *_with_device("iqgpu_chain_dcagc_dc_measure_range", C.c_int, [_vp, C.c_uint64, _vp, _sz, _sz, _vp, _sz, C.POINTER(_sz), _vp]),
    *_with_device("iqgpu_chain_dcrms_dc_measure_range", C.c_int, [_vp, C.c_uint64, _vp, _sz, _sz, _vp, _sz, C.POINTER(_sz), _vp]),
    ("iqgpu_dc_measure_range_launch_entries", _sz, []),
    ("iqgpu_design_state_size", C.c_int, [C.POINTER(ChainDesc), C.POINTER(_sz)]),
    ("iqgpu_state_inspect", C.c_int, [_vp, _sz, C.POINTER(StateInfo)]),
    ("iqgpu_chain_tell", C.c_int, [_vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    ("iqgpu_chain_save_state", C.c_int, [_vp, _vp, _sz, C.POINTER(_sz)]),
    ("iqgpu_chain_load_state", C.c_int, [_vp, _vp, _sz]),
    ("iqgpu_chain_set_iq_factors", C.c_int, [_vp, C.c_float, C.c_float]),
    ("iqgpu_chain_max_out_frames", _sz, [_vp, _sz]),
    ("iqgpu_chain_next_out_frames", _sz, [_vp, _sz]),
    ("iqgpu_iq_optimizer_create", C.c_int, [C.POINTER(_vp)]),
    ("iqgpu_iq_optimizer_destroy", None, [_vp]),
    ("iqgpu_iq_optimizer_seed", C.c_int, [_vp, C.c_uint32]),
    ("iqgpu_iq_optimizer_set_rng", C.c_int, [_vp, RAND_DIR_FN, _vp]),
    ("iqgpu_iq_optimizer_set_factors", C.c_int, [_vp, C.c_float, C.c_float]),
    ("iqgpu_iq_optimizer_get_factors", C.c_int, [_vp, C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    ("iqgpu_iq_optimizer_get_stats", C.c_int, [_vp, C.POINTER(IqOptimizerStats)]),
    ("iqgpu_iq_optimizer_metric", C.c_float, [_vp, _vp, C.c_float, C.c_float]),
    ("iqgpu_iq_optimizer_run", C.c_int, [_vp, _vp, C.c_double, C.POINTER(C.c_int)]),
    ("iqgpu_iq_optimizer_touch", C.c_int, [_vp, C.c_double]),
    ("iqgpu_chain_enable_iq_probe", C.c_int, [_vp, C.c_int]),
    ("iqgpu_chain_read_iq_probe", C.c_int, [_vp, _vp, C.POINTER(C.c_int)]),
    ("iqgpu_iq_optimizer_service", C.c_int, [_vp, _vp, C.c_double, C.POINTER(C.c_int)]),
    ("iqgpu_iq_calib_opts_init", None, [C.POINTER(IqCalibOpts)]),
    ("iqgpu_iq_metric_batch", C.c_int, [C.c_int, _vp, _sz, _sz, _vp, _sz, _vp, _vp]),
    ("iqgpu_iq_metric_batch_device", C.c_int, [C.c_int, _vp, _sz, _sz, _vp, _sz, _vp, _vp, _vp]),
    ("iqgpu_iq_metric_geometry", None, [C.POINTER(_sz), C.POINTER(_sz)]),
    ("iqgpu_iq_optimizer_calibrate", C.c_int, [_vp, _vp, _sz, _sz, C.POINTER(IqCalibOpts), C.POINTER(IqCalibReport)]),
    *_with_device("iqgpu_chain_calibrate_iq", C.c_int, [_vp, _vp, _sz, C.POINTER(IqCalibOpts), C.POINTER(IqCalibReport)]),
    *_with_device("iqgpu_chain_calibrate_iq_blocks", C.c_int, [_vp, _vp, _sz, C.c_uint32, _vp, _sz, C.POINTER(_sz)]),
    ("iqgpu_psd_opts_init", None, [C.POINTER(PsdOpts)]),
    ("iqgpu_psd_window", C.c_int, [C.POINTER(PsdOpts), _vp, _sz, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    ("iqgpu_psd_segments", C.c_int, [C.POINTER(PsdOpts), C.c_uint64, C.POINTER(C.c_uint64)]),
    ("iqgpu_psd_geometry", None, [C.POINTER(_sz)]),
    ("iqgpu_psd_create", C.c_int, [C.c_int, C.c_int, C.POINTER(PsdOpts), C.POINTER(_vp)]),
    ("iqgpu_psd_destroy", None, [_vp]),
    ("iqgpu_psd_reset", C.c_int, [_vp]),
    ("iqgpu_psd_push", C.c_int, [_vp, _vp, _sz]),
    ("iqgpu_psd_push_device", C.c_int, [_vp, _vp, _sz, _vp]),
    ("iqgpu_psd_read", C.c_int, [_vp, _vp, _vp, C.POINTER(PsdInfo)]),
    ("iqgpu_sgram_opts_init", None, [C.POINTER(SgramOpts)]),
    ("iqgpu_sgram_rows", C.c_int, [C.POINTER(SgramOpts), C.c_uint64, C.POINTER(C.c_uint64)]),
    ("iqgpu_sgram_create", C.c_int, [C.c_int, C.c_int, C.POINTER(SgramOpts), C.POINTER(_vp)]),
    ("iqgpu_sgram_destroy", None, [_vp]),
    ("iqgpu_sgram_reset", C.c_int, [_vp]),
    ("iqgpu_sgram_max_rows", _sz, [_vp, _sz]),
    ("iqgpu_sgram_push", C.c_int, [_vp, _vp, _sz, _vp, _vp, _sz, C.POINTER(_sz)]),
    ("iqgpu_sgram_push_device", C.c_int, [_vp, _vp, _sz, _vp, _vp, _sz, C.POINTER(_sz), _vp]),
    ("iqgpu_sgram_read_open", C.c_int, [_vp, _vp, _vp, C.POINTER(SgramInfo)]),
    ("iqgpu_stats_geometry", None, [C.POINTER(_sz)]),
    ("iqgpu_stats_create", C.c_int, [C.c_int, C.c_int, C.POINTER(_vp)]),
    ("iqgpu_stats_destroy", None, [_vp]),
    ("iqgpu_stats_reset", C.c_int, [_vp]),
    ("iqgpu_stats_push", C.c_int, [_vp, _vp, _sz]),
    ("iqgpu_stats_push_device", C.c_int, [_vp, _vp, _sz, _vp]),
    ("iqgpu_stats_read", C.c_int, [_vp, C.POINTER(StatsResult)]),
    ("iqgpu_stats_merge", C.c_int, [C.POINTER(StatsResult), C.POINTER(StatsResult)]),
    ("iqgpu_stats_derive", C.c_int, [C.POINTER(StatsResult), C.POINTER(StatsDerived)]),
    ("iqgpu_env_opts_init", None, [C.POINTER(EnvOpts)]),
    ("iqgpu_env_rows", C.c_int, [C.POINTER(EnvOpts), C.c_uint64, C.POINTER(C.c_uint64)]),
    ("iqgpu_env_create", C.c_int, [C.c_int, C.c_int, C.POINTER(EnvOpts), C.POINTER(_vp)]),
    ("iqgpu_env_destroy", None, [_vp]),
    ("iqgpu_env_reset", C.c_int, [_vp]),
    ("iqgpu_env_max_rows", _sz, [_vp, _sz]),
    ("iqgpu_env_push", C.c_int, [_vp, _vp, _sz, _vp, _vp, _vp, _sz, C.POINTER(_sz)]),
    ("iqgpu_env_push_device", C.c_int, [_vp, _vp, _sz, _vp, _vp, _vp, _sz, C.POINTER(_sz), _vp]),
    ("iqgpu_env_read_open", C.c_int, [_vp, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_uint32), C.POINTER(EnvInfo)]),
    ("iqgpu_env_bursts", C.c_int, [_vp, _sz, C.POINTER(EnvBurstOpts), _vp, _sz, C.POINTER(_sz)]),
    ("iqgpu_env_floor", C.c_int, [_vp, _sz, C.c_uint32, C.c_double, C.POINTER(C.c_double)]),
    ("iqgpu_lag_opts_init", None, [C.POINTER(LagOpts)]),
    ("iqgpu_lag_rows", C.c_int, [C.POINTER(LagOpts), C.c_uint64, C.POINTER(C.c_uint64)]),
    ("iqgpu_lag_create", C.c_int, [C.c_int, C.c_int, C.POINTER(LagOpts), C.POINTER(_vp)]),
    ("iqgpu_lag_destroy", None, [_vp]),
    ("iqgpu_lag_reset", C.c_int, [_vp]),
    ("iqgpu_lag_max_rows", _sz, [_vp, _sz]),
    ("iqgpu_lag_push", C.c_int, [_vp, _vp, _sz, _vp, _vp, _sz, C.POINTER(_sz)]),
    ("iqgpu_lag_push_device", C.c_int, [_vp, _vp, _sz, _vp, _vp, _sz, C.POINTER(_sz), _vp]),
    ("iqgpu_lag_read_open", C.c_int, [_vp, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(LagInfo)]),
    ("iqgpu_lag_freq", C.c_int, [C.c_double, C.c_double, C.c_uint32, C.c_double, C.POINTER(C.c_double)]),
    ("iqgpu_lag_estimate_rows", C.c_int, [_vp, _vp, _sz, C.POINTER(LagOpts), C.c_uint32, _sz, _sz, C.c_double, C.POINTER(LagEstimate)]),
    ("iqgpu_match_opts_init", None, [C.POINTER(MatchOpts)]),
    ("iqgpu_match_rows", C.c_int, [C.POINTER(MatchOpts), C.c_uint64, C.POINTER(C.c_uint64)]),
    ("iqgpu_match_create", C.c_int, [C.c_int, C.c_int, C.POINTER(MatchOpts), _vp, C.POINTER(_vp)]),
    ("iqgpu_match_destroy", None, [_vp]),
    ("iqgpu_match_reset", C.c_int, [_vp]),
    ("iqgpu_match_max_rows", _sz, [_vp, _sz]),
    ("iqgpu_match_push", C.c_int, [_vp, _vp, _sz, _vp, _vp, _vp, _sz, C.POINTER(_sz)]),
    ("iqgpu_match_push_device", C.c_int, [_vp, _vp, _sz, _vp, _vp, _vp, _sz, C.POINTER(_sz), _vp]),
    ("iqgpu_match_read_open", C.c_int, [_vp, _vp, _vp, _vp, C.POINTER(MatchInfo)]),
    ("iqgpu_match_shift_bank", C.c_int, [_vp, C.c_uint32, _vp, C.c_uint32, C.c_double, _vp]),
    ("iqgpu_match_peaks", C.c_int, [_vp, _vp, _vp, _sz, C.POINTER(MatchOpts), C.c_double, _vp, _sz, C.POINTER(_sz)]),
    ("iqgpu_wav_info_init", None, [C.POINTER(WavInfo)]),
    ("iqgpu_wav_parse_auxi", C.c_int, [_vp, _sz, C.POINTER(WavInfo)]),
    ("iqgpu_wav_parse_filename", C.c_int, [C.c_char_p, C.POINTER(WavInfo)]),
    ("iqgpu_wav_probe", C.c_int, [C.c_char_p, C.POINTER(WavInfo)]),
    ("iqgpu_wav_shift_hz", C.c_int, [C.POINTER(WavInfo), C.c_float, C.c_float, C.POINTER(C.c_double)]),
    ("iqgpu_chain_set_stream", C.c_int, [_vp, _vp]),
    ("iqgpu_chain_get_stream", _vp, [_vp]),
    ("iqgpu_chain_synchronize", C.c_int, [_vp]),
    ("iqgpu_chain_set_profiling", C.c_int, [_vp, C.c_int]),
    ("iqgpu_chain_get_profile", C.c_int, [_vp, C.POINTER(Profile)]),
    ("iqgpu_chain_front_kernel", C.c_char_p, [_vp]),
    ("iqgpu_debug_set", C.c_int, [C.c_char_p, C.c_char_p]),
    ("iqgpu_debug_list", C.c_int, [C.c_char_p, _sz]),
    ("iqgpu_chain_debug_read_scratch", C.c_int, [_vp, _vp]),
    ("iqgpu_get_bytes_per_sample", _sz, [C.c_int]),
    ("iqgpu_convert_block_to_cf32", C.c_int, [_vp, _vp, _sz, C.c_int, C.c_float, C.c_int]),
    ("iqgpu_convert_cf32_to_block", C.c_int, [_vp, _vp, _sz, C.c_int, C.c_int]),
    ("iqgpu_device_malloc", C.c_int, [C.c_int, _sz, C.POINTER(_vp)]),
    ("iqgpu_device_free", C.c_int, [C.c_int, _vp]),
    ("iqgpu_host_malloc_pinned", C.c_int, [_sz, C.POINTER(_vp)]),
    ("iqgpu_host_free_pinned", C.c_int, [_vp]),
    ("iqgpu_memcpy_h2d", C.c_int, [C.c_int, _vp, _vp, _sz]),
    ("iqgpu_memcpy_d2h", C.c_int, [C.c_int, _vp, _vp, _sz]),
    ("iqgpu_memcpy_h2d_async", C.c_int, [_vp, _vp, _sz, _vp]),
    ("iqgpu_memcpy_d2h_async", C.c_int, [_vp, _vp, _sz, _vp]),
    ("iqgpu_stream_create", C.c_int, [C.c_int, C.POINTER(_vp)]),
    ("iqgpu_stream_destroy", C.c_int, [_vp]),
    ("iqgpu_stream_synchronize", C.c_int, [_vp]),
    ("iqgpu_event_create", C.c_int, [C.POINTER(_vp)]),
    ("iqgpu_event_destroy", C.c_int, [_vp]),
    ("iqgpu_event_record", C.c_int, [_vp, _vp]),
    ("iqgpu_stream_wait_event", C.c_int, [_vp, _vp]),
    ("iqgpu_event_elapsed_ms", C.c_int, [_vp, _vp, C.POINTER(C.c_float)]),
]

_lib = None


def load():
    """Returns the loaded library; raises if libiqgpu.so has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                "libiqgpu.so is missing at %s -- run `python -m iq_tool_amd.build` (needs hipcc). "
                "iq_tool_amd has no CPU fallback." % LIB_PATH)
        lib = C.CDLL(LIB_PATH)
        for name, res, args in SYMBOLS:
            fn = getattr(lib, name)          # AttributeError if the ABI lost a symbol
            fn.restype = res
            fn.argtypes = args
        _lib = lib
    return _lib


# The library reads no switch from the environment (ABI v6: iqgpu_debug_set).  The tests, bench.py and the A/B scripts under tools/
# select kernels with IQGPU_<NAME>=... variables of THEIR OWN process; this mirror forwards them -- explicitly, right before a
# chain is designed or created -- so that `IQGPU_NO_FAST=1 python bench.py` keeps working while a host that links libiqgpu sees
# no environment dependence at all.
DEBUG_NAMES = ("force_generic", "no_fast", "agc_nofuse", "no_raw0", "no_kt", "fft_no_r16", "no_fat", "force_fat", "fat", "mid8",
               "no_s2", "no_fused_move", "no_p0", "no_casc2", "no_mid_8bit", "fuse_filter", "tap_fold", "steal", "steal_min",
               "steal_rounds", "steal_stride", "steal_lanes", "run_weights", "cus", "fft_log2n", "fft_threads", "fft_geometry", "casc2_min_run",
               "sysfs_root", "nco_hold", "measure_route", "dc_range_slice_frames")
_forwarded = set()      # names whose switch apply_debug_env set from the environment and has not cleared since


def apply_debug_env():
    """forwards this process's IQGPU_<NAME> variables to the library's diagnostic switches: an exported variable sets its switch,
    one that went away clears the switch it had set, and every other switch (set directly through iqgpu_debug_set) stays.  The
    table is never cleared as a whole, so concurrent calls under the same environment agree and no caller sees it emptied."""
    lib = load()
    for name in DEBUG_NAMES:
        v = os.environ.get("IQGPU_" + name.upper())
        if v:
            check(lib.iqgpu_debug_set(name.encode(), v.encode()))
            _forwarded.add(name)
        elif name in _forwarded:
            check(lib.iqgpu_debug_set(name.encode(), None))
            _forwarded.discard(name)


def debug_switches():
    """what iqgpu_debug_list reports: {name: value} of the switches that are set"""
    buf = C.create_string_buffer(4096)
    check(load().iqgpu_debug_list(buf, len(buf)))
    return dict(kv.split("=", 1) for kv in buf.value.decode().split(";") if kv)


def check(rc):
    if rc != 0:
        raise IqgpuError(rc, load().iqgpu_last_error().decode("utf-8", "replace"))
