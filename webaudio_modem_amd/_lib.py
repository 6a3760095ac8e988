"""ctypes loader for libfskhip.so (the C ABI in include/fskhip.h and include/fskhip_next.h).

There is no fallback of any kind: if the HIP extension is missing this raises, and every
compute entry point fails with FSKHIP_E_NO_DEVICE when no GPU is present.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libfskhip.so")   # (measurement tools load other builds by setting this before lib() runs)

MAX_PATTERN_BYTES = 16
OK = 0
E_INVALID, E_NOT_CONFIGURED, E_UNSUPPORTED, E_NO_DEVICE, E_HIP, E_NOMEM, E_OVERFLOW, E_BUSY, E_HANDOFF = -1, -2, -3, -4, -5, -6, -7, -8, -9
PROC_CLEAR_RX_ON_TX_COMPLETE, PROC_GRAPH = 1, 2
PROC_RATECVT_PAIR = 4      # (a ratecvt quantum's TX side through the two launches its fused kernel replaces: measurements, tests)
XM_NEED_MORE, XM_EOT, XM_TRUNCATED, XM_INVALID_SEQUENCE, XM_INVALID_CRC, XM_UNEXPECTED_SEQUENCE = 0, 1, 2, 3, 4, 5
XT_IDLE, XT_WAIT_NAK, XT_WAIT_ACK, XT_WAIT_FINAL_ACK = 0, 1, 2, 3
XT_PROGRESS, XT_DONE, XT_MAX_RETRIES, XT_ABORTED = 0, 1, 2, 3
XR_IDLE, XR_SEND_NAK, XR_WAIT_BLOCK, XR_SEND_ACK = 0, 1, 2, 3
XR_PROGRESS, XR_DONE, XR_MAX_RETRIES, XR_ABORTED, XR_FILE_FULL = 0, 1, 2, 3, 4
PRECISION_F32, PRECISION_F64 = 0, 1
DEMOD_WRITEBACK_AGC = 1
SAMPLES_F32, SAMPLES_S16, SAMPLES_MULAW, SAMPLES_ALAW = 0, 1, 2, 3
LAYOUT_STREAM_MAJOR, LAYOUT_SAMPLE_MAJOR = 0, 1
RESAMPLE_UP, RESAMPLE_DOWN = 0, 1
RATECVT_CAPTURE, RATECVT_PLAYBACK = 0, 1


class Config(C.Structure):
    """fskhip_config == FSKConfig (reference src/modems/fsk.ts:5-17)."""
    _fields_ = [
        ("sampleRate", C.c_double), ("baudRate", C.c_double),
        ("markFrequency", C.c_double), ("spaceFrequency", C.c_double),
        ("preamblePattern", C.c_int32 * MAX_PATTERN_BYTES), ("preambleLen", C.c_int32),
        ("sfdPattern", C.c_int32 * MAX_PATTERN_BYTES), ("sfdLen", C.c_int32),
        ("startBits", C.c_int32), ("stopBits", C.c_int32), ("parity", C.c_int32),
        ("syncThreshold", C.c_double), ("agcEnabled", C.c_int32),
        ("preFilterBandwidth", C.c_double), ("adaptiveThreshold", C.c_int32),
    ]


class SignalQuality(C.Structure):
    """fskhip_signal_quality (include/fskhip.h): opt-in estimates; the reference's getSignalQuality() is all zeros"""
    _fields_ = [(k, C.c_double) for k in ("snr", "ber", "eyeOpening", "phaseJitter", "frequencyOffset",
                                          "signalLevel", "noiseFloor", "frames", "bytes")]


class Status(C.Structure):
    """fskhip_status == getStatus() (fsk.ts:481-493) + agcGain + eodCount."""
    _fields_ = [
        ("ready", C.c_int32), ("frameStarted", C.c_int32),
        ("globalSampleCounter", C.c_double), ("receivedBitsLength", C.c_double),
        ("byteBufferLength", C.c_double), ("demodulationCalls", C.c_double),
        ("syncDetections", C.c_double), ("silenceThreshold", C.c_double),
        ("totalSamplesProcessed", C.c_double), ("agcGain", C.c_double), ("eodCount", C.c_double),
    ]


class SnapshotInfo(C.Structure):
    """fskhip_snapshot_info (include/fskhip.h): what a stream snapshot holds"""
    _fields_ = [("n_streams", C.c_uint32), ("precision", C.c_int32), ("per_stream_configs", C.c_uint32), ("record_bytes", C.c_uint32),
                ("demodulationCalls", C.c_double), ("totalSamplesProcessed", C.c_double)]


class ProcessorSnapshotInfo(C.Structure):
    """fskhip_processor_snapshot_info (include/fskhip_next.h): what a processor snapshot holds"""
    _fields_ = [("n_streams", C.c_uint32), ("rx_capacity", C.c_uint32), ("payload_capacity", C.c_uint32), ("record_bytes", C.c_uint32)]


class XModemSnapshotInfo(C.Structure):
    """fskhip_xmodem_snapshot_info (include/fskhip_next.h): what an XModem snapshot holds"""
    _fields_ = [("kind", C.c_uint32), ("n_streams", C.c_uint32), ("param0", C.c_uint32), ("param1", C.c_uint32), ("file_bytes", C.c_uint64)]


class XModemTimerSnapshotInfo(C.Structure):
    """fskhip_xmodem_timer_snapshot_info (include/fskhip_next.h): what an XModem timer snapshot holds"""
    _fields_ = [("kind", C.c_uint32), ("n_streams", C.c_uint32), ("timeout_samples", C.c_uint32), ("reserved", C.c_uint32)]


class ResamplerSnapshotInfo(C.Structure):
    """fskhip_resampler_snapshot_info (include/fskhip_next.h): what a resampler snapshot holds"""
    _fields_ = [("n_streams", C.c_uint32), ("direction", C.c_int), ("factor", C.c_uint32), ("n_taps", C.c_uint32), ("precision", C.c_int),
                ("history", C.c_uint32)]


class RatecvtSnapshotInfo(C.Structure):
    """fskhip_ratecvt_snapshot_info (include/fskhip_next.h): what a rate converter snapshot holds"""
    _fields_ = [("n_streams", C.c_uint32), ("direction", C.c_int), ("up", C.c_uint32), ("down", C.c_uint32), ("n_taps", C.c_uint32), ("precision", C.c_int),
                ("history", C.c_uint32), ("position", C.c_uint32)]


class XModemResult(C.Structure):
    """fskhip_xmodem_result (include/fskhip_next.h)."""
    _fields_ = [
        ("status", C.c_uint32), ("expected_after", C.c_uint32), ("packets", C.c_uint32), ("dropped", C.c_uint32),
        ("consumed", C.c_uint32), ("data_len", C.c_uint32), ("err_seq", C.c_int32), ("err_len", C.c_int32),
        ("crc_rx", C.c_int32), ("crc_calc", C.c_int32),
    ]


class XModemTxEvent(C.Structure):
    """fskhip_xmodem_tx_event (include/fskhip_next.h)."""
    _fields_ = [
        ("status", C.c_uint32), ("state_after", C.c_uint32), ("control", C.c_int32), ("sent_len", C.c_uint32),
        ("sequence", C.c_uint32), ("fragment_index", C.c_uint32), ("n_fragments", C.c_uint32), ("retries", C.c_uint32),
    ]


class XModemRecvEvent(C.Structure):
    """fskhip_xmodem_recv_event (include/fskhip_next.h)."""
    _fields_ = [
        ("status", C.c_uint32), ("state_after", C.c_uint32), ("control", C.c_int32), ("step", C.c_uint32),
        ("seq", C.c_int32), ("len", C.c_int32), ("accepted_len", C.c_uint32), ("file_len", C.c_uint32),
        ("expected", C.c_uint32), ("retries", C.c_uint32), ("crc_rx", C.c_int32), ("crc_calc", C.c_int32),
    ]


# every symbol include/*.h declares: (name, restype, argtypes)
_P = C.c_void_p
_SYMBOLS = [
    ("fskhip_default_config", None, [C.POINTER(Config)]),
    ("fskhip_create", C.c_int, [C.POINTER(Config), C.c_uint32, C.c_uint32, C.c_int, C.c_int, C.POINTER(_P)]),
    ("fskhip_destroy", C.c_int, [_P]),
    ("fskhip_n_streams", C.c_uint32, [_P]),
    ("fskhip_max_bytes", C.c_size_t, [_P, C.c_size_t]),
    ("fskhip_last_kernel", C.c_char_p, [_P]),
    ("fskhip_blk_lanes", C.c_uint32, [_P]),
    ("fskhip_demodulate_host", C.c_int, [_P, _P, C.c_size_t, C.c_size_t, _P, C.c_size_t, _P, _P, C.c_uint32]),
    ("fskhip_demodulate_device", C.c_int, [_P, _P, C.c_size_t, C.c_size_t, _P, C.c_size_t, _P, _P, C.c_uint32, _P]),
    ("fskhip_sample_bytes", C.c_size_t, [C.c_int]),
    ("fskhip_ingest_device", C.c_int, [_P, C.c_int, C.c_int, C.c_uint32, C.c_size_t, C.c_size_t, _P, C.c_size_t, _P]),
    ("fskhip_demodulate_host_fmt", C.c_int, [_P, _P, C.c_int, C.c_int, C.c_size_t, C.c_size_t, _P, C.c_size_t, _P, _P, C.c_uint32]),
    ("fskhip_egress_device", C.c_int, [_P, C.c_size_t, _P, C.c_uint32, C.c_size_t, C.c_int, C.c_int, _P, C.c_size_t, _P]),
    ("fskhip_modulate_host_fmt", C.c_int, [_P, _P, _P, C.c_size_t, C.c_int, C.c_int, _P, C.c_size_t, C.c_size_t, _P]),
    ("fskhip_modulated_length", C.c_size_t, [_P, C.c_size_t]),
    ("fskhip_modulate_host", C.c_int, [_P, _P, _P, C.c_size_t, _P, C.c_size_t, _P]),
    ("fskhip_modulate_device", C.c_int, [_P, _P, _P, C.c_size_t, _P, C.c_size_t, _P, _P]),
    ("fskhip_reset", C.c_int, [_P, C.c_int64]),
    ("fskhip_get_status", C.c_int, [_P, C.c_uint32, C.POINTER(Status)]),
    ("fskhip_get_faults", C.c_int, [_P, C.c_void_p, C.POINTER(C.c_uint32)]),
    ("fskhip_synth_device", C.c_int, [_P, _P, C.c_size_t, C.c_size_t, C.c_uint32, C.c_uint64, C.c_uint32,
                                      C.c_double, C.c_double, _P]),
    ("fskhip_synth_payload_byte", C.c_uint8, [C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32]),
    ("fskhip_synth_stream_params", None, [C.c_uint64, C.c_uint32, C.c_uint32, C.c_double, C.c_double,
                                          C.POINTER(C.c_uint32), C.POINTER(C.c_double)]),
    ("fskhip_add_awgn_device", C.c_int, [_P, _P, C.c_size_t, C.c_size_t, C.c_double, C.c_uint64, _P]),
    ("fskhip_demod_supported", C.c_int, [_P]),
    ("fskhip_trace_enable", C.c_int, [_P, C.c_int64, C.c_size_t]),
    ("fskhip_trace_read_pre", C.c_int, [_P, _P, C.c_size_t, C.POINTER(C.c_size_t)]),
    ("fskhip_trace_read", C.c_int, [_P, _P, _P, _P, C.c_size_t, C.POINTER(C.c_size_t)]),
    ("fskhip_probe_read_device", C.c_int, [_P, _P, C.c_size_t, C.c_size_t, _P]),
    ("fskhip_butterworth_lowpass", None, [C.c_double, C.c_double, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    ("fskhip_butterworth_highpass", None, [C.c_double, C.c_double, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    ("fskhip_butterworth_bandpass", None, [C.c_double, C.c_double, C.c_double, C.POINTER(C.c_double),
                                           C.POINTER(C.c_double)]),
    ("fskhip_carry_over", C.c_int, [_P, _P]),
    ("fskhip_remap_streams", C.c_int, [_P, _P, _P, C.c_uint32]),
    ("fskhip_snapshot_bytes", C.c_size_t, [_P, C.c_uint32]),
    ("fskhip_snapshot_streams", C.c_int, [_P, _P, C.c_uint32, _P, C.c_size_t, C.POINTER(C.c_size_t)]),
    ("fskhip_snapshot_info_get", C.c_int, [_P, C.c_size_t, C.POINTER(SnapshotInfo)]),
    ("fskhip_snapshot_stream_config", C.c_int, [_P, C.c_size_t, C.c_uint32, C.POINTER(Config)]),
    ("fskhip_snapshot_concat", C.c_int, [C.POINTER(_P), C.POINTER(C.c_size_t), C.c_uint32, _P, C.c_size_t, C.POINTER(C.c_size_t)]),
    ("fskhip_restore_streams", C.c_int, [_P, _P, C.c_size_t, _P, C.c_uint32]),
    ("fskhip_enable_signal_quality", C.c_int, [_P, C.c_int]),
    ("fskhip_get_signal_quality", C.c_int, [_P, C.c_uint32, C.POINTER(SignalQuality)]),
    ("fskhip_host_alloc", C.c_int, [C.c_size_t, C.POINTER(_P)]),
    ("fskhip_host_free", C.c_int, [_P]),
    ("fskhip_device_malloc", C.c_int, [_P, C.c_size_t, C.POINTER(_P)]),
    ("fskhip_device_free", C.c_int, [_P, _P]),
    ("fskhip_memcpy_h2d", C.c_int, [_P, _P, _P, C.c_size_t]),
    ("fskhip_memcpy_d2h", C.c_int, [_P, _P, _P, C.c_size_t]),
    ("fskhip_synchronize", C.c_int, [_P]),
    ("fskhip_set_option", C.c_int, [_P, C.c_char_p, C.c_char_p]),
    ("fskhip_debug_state", C.c_int, [_P, C.c_uint32, C.POINTER(C.c_double), C.c_uint32, C.POINTER(C.c_uint32), C.c_uint32,
                                     C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    ("fskhip_clock_probe_begin", C.c_int, [_P, C.c_double]),
    ("fskhip_clock_probe_end", C.c_int, [_P, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    ("fskhip_timing_begin", C.c_int, [_P]),
    ("fskhip_timing_end", C.c_int, [_P, C.POINTER(C.c_uint32), C.POINTER(C.c_double)]),
    ("fskhip_last_error", C.c_char_p, []),
    ("fskhip_abi_version", C.c_int, []),
    ("fskhip_device_count", C.c_int, []),
    # ---- include/fskhip_next.h ----
    ("fskhip_crc16_device", C.c_int, [_P, C.c_size_t, _P, C.c_uint32, _P, _P]),
    ("fskhip_crc16_host", C.c_int, [C.c_int, _P, C.c_size_t, _P, C.c_uint32, _P]),
    ("fskhip_xmodem_serialize_device", C.c_int, [_P, C.c_size_t, _P, _P, C.c_uint32, _P, C.c_size_t, _P, _P]),
    ("fskhip_xmodem_serialize_host", C.c_int, [C.c_int, _P, C.c_size_t, _P, _P, C.c_uint32, _P, C.c_size_t, _P]),
    ("fskhip_xmodem_scan_device", C.c_int, [_P, C.c_size_t, _P, _P, C.c_uint32, _P, C.c_size_t, _P, _P]),
    ("fskhip_xmodem_scan_host", C.c_int, [C.c_int, _P, C.c_size_t, _P, _P, C.c_uint32, _P, C.c_size_t, _P]),
    ("fskhip_processor_create", C.c_int, [_P, C.c_uint32, C.POINTER(_P)]),
    ("fskhip_processor_destroy", C.c_int, [_P]),
    ("fskhip_processor_process_device", C.c_int, [_P, _P, C.c_size_t, C.c_size_t, _P, C.c_size_t, C.c_size_t, C.c_uint32, _P]),
    ("fskhip_processor_process_host", C.c_int, [_P, _P, C.c_size_t, C.c_size_t, _P, C.c_size_t, C.c_size_t, C.c_uint32]),
    ("fskhip_processor_graph_stats", C.c_int, [_P, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    ("fskhip_processor_last_tx_kernel", C.c_char_p, [_P]),
    ("fskhip_processor_process_fmt_device", C.c_int, [_P, _P, C.c_int, C.c_int, C.c_size_t, C.c_size_t, _P, C.c_int, C.c_int, C.c_size_t, C.c_size_t, C.c_uint32, _P]),
    ("fskhip_processor_process_fmt_host", C.c_int, [_P, _P, C.c_int, C.c_int, C.c_size_t, C.c_size_t, _P, C.c_int, C.c_int, C.c_size_t, C.c_size_t, C.c_uint32]),
    ("fskhip_processor_modulate_host", C.c_int, [_P, _P, _P, C.c_size_t, _P]),
    ("fskhip_processor_tx_state_host", C.c_int, [_P, _P, _P, _P, _P]),
    ("fskhip_processor_rx_drain_host", C.c_int, [_P, _P, C.c_size_t, _P]),
    ("fskhip_processor_rx_drain_sparse_host", C.c_int, [_P, _P, C.c_uint32, _P, _P, C.c_uint32, _P, C.c_size_t, _P, _P]),
    ("fskhip_processor_rx_drain_sparse_device", C.c_int, [_P, _P, C.c_uint32, _P, _P, C.c_uint32, _P, C.c_size_t, _P, _P]),
    ("fskhip_processor_rx_length_host", C.c_int, [_P, _P]),
    ("fskhip_processor_reset", C.c_int, [_P, C.c_int64]),
    ("fskhip_processor_remap", C.c_int, [_P, _P, _P, C.c_uint32]),
    ("fskhip_processor_snapshot_bytes", C.c_size_t, [_P, _P, C.c_uint32]),
    ("fskhip_processor_snapshot", C.c_int, [_P, _P, C.c_uint32, _P, C.c_size_t, C.POINTER(C.c_size_t)]),
    ("fskhip_processor_snapshot_info_get", C.c_int, [_P, C.c_size_t, C.POINTER(ProcessorSnapshotInfo)]),
    ("fskhip_processor_snapshot_concat", C.c_int, [C.POINTER(_P), C.POINTER(C.c_size_t), C.c_uint32, _P, C.c_size_t, C.POINTER(C.c_size_t)]),
    ("fskhip_processor_restore", C.c_int, [_P, _P, C.c_size_t, _P, C.c_uint32]),
    ("fskhip_xmodem_rx_create", C.c_int, [_P, C.POINTER(_P)]),
    ("fskhip_xmodem_rx_destroy", C.c_int, [_P]),
    ("fskhip_xmodem_rx_reset", C.c_int, [_P, C.c_int64]),
    ("fskhip_xmodem_rx_state_get", C.c_int, [_P, _P, _P, _P]),
    ("fskhip_xmodem_rx_state_set", C.c_int, [_P, _P, _P, _P]),
    ("fskhip_xmodem_rx_poll_host", C.c_int, [_P, _P, _P, _P, _P, C.c_uint32, _P, C.c_size_t, _P, _P]),
    ("fskhip_xmodem_rx_poll_device", C.c_int, [_P, _P, _P, _P, _P, C.c_uint32, _P, C.c_size_t, _P, _P]),
    ("fskhip_xmodem_tx_create", C.c_int, [_P, C.c_uint32, C.c_uint32, C.POINTER(_P)]),
    ("fskhip_xmodem_tx_destroy", C.c_int, [_P]),
    ("fskhip_xmodem_tx_send_host", C.c_int, [_P, _P, _P, _P]),
    ("fskhip_xmodem_tx_poll_host", C.c_int, [_P, _P, _P, _P, _P, C.c_uint32, _P]),
    ("fskhip_xmodem_tx_poll_device", C.c_int, [_P, _P, _P, _P, _P, C.c_uint32, _P, _P]),
    ("fskhip_xmodem_tx_state_get", C.c_int, [_P, _P, _P, _P, _P, _P, _P]),
    ("fskhip_xmodem_tx_state_set", C.c_int, [_P, _P, _P, _P, _P, _P, _P]),
    ("fskhip_xmodem_tx_reset", C.c_int, [_P, C.c_int64]),
    ("fskhip_xmodem_recv_create", C.c_int, [_P, C.c_uint32, C.c_uint32, C.POINTER(_P)]),
    ("fskhip_xmodem_recv_destroy", C.c_int, [_P]),
    ("fskhip_xmodem_recv_start_host", C.c_int, [_P, _P]),
    ("fskhip_xmodem_recv_poll_host", C.c_int, [_P, _P, _P, _P, _P, _P, C.c_uint32, _P]),
    ("fskhip_xmodem_recv_poll_device", C.c_int, [_P, _P, _P, _P, _P, _P, C.c_uint32, _P, _P]),
    ("fskhip_xmodem_recv_state_get", C.c_int, [_P, _P, _P, _P, _P, _P, _P, _P]),
    ("fskhip_xmodem_recv_state_set", C.c_int, [_P, _P, _P, _P, _P, _P, _P, _P]),
    ("fskhip_xmodem_recv_reset", C.c_int, [_P, C.c_int64]),
    ("fskhip_xmodem_recv_files_host", C.c_int, [_P, _P, C.c_uint32, _P, _P, C.c_size_t, _P]),
    ("fskhip_xmodem_recv_files_set_host", C.c_int, [_P, _P, C.c_uint32, _P, _P]),
    ("fskhip_xmodem_timer_create_recv", C.c_int, [_P, C.c_uint32, C.POINTER(_P)]),
    ("fskhip_xmodem_timer_create_tx", C.c_int, [_P, C.c_uint32, C.POINTER(_P)]),
    ("fskhip_xmodem_timer_destroy", C.c_int, [_P]),
    ("fskhip_xmodem_timer_reset", C.c_int, [_P, C.c_int64]),
    ("fskhip_xmodem_timer_state_get", C.c_int, [_P, _P, _P]),
    ("fskhip_xmodem_timer_state_set", C.c_int, [_P, _P, _P]),
    ("fskhip_xmodem_recv_poll_timed_host", C.c_int, [_P, C.c_uint32, _P, _P, _P, _P, C.c_uint32, _P]),
    ("fskhip_xmodem_recv_poll_timed_device", C.c_int, [_P, C.c_uint32, _P, _P, _P, _P, C.c_uint32, _P, _P]),
    ("fskhip_xmodem_tx_poll_timed_host", C.c_int, [_P, C.c_uint32, _P, _P, _P, _P, C.c_uint32, _P]),
    ("fskhip_xmodem_tx_poll_timed_device", C.c_int, [_P, C.c_uint32, _P, _P, _P, _P, C.c_uint32, _P, _P]),
    ("fskhip_xmodem_timer_snapshot_info_get", C.c_int, [_P, C.c_size_t, C.POINTER(XModemTimerSnapshotInfo)]),
    ("fskhip_xmodem_timer_remap", C.c_int, [_P, _P, _P, C.c_uint32]),
    ("fskhip_xmodem_timer_snapshot_bytes", C.c_size_t, [_P, _P, C.c_uint32]),
    ("fskhip_xmodem_timer_snapshot", C.c_int, [_P, _P, C.c_uint32, _P, C.c_size_t, C.POINTER(C.c_size_t)]),
    ("fskhip_xmodem_timer_restore", C.c_int, [_P, _P, C.c_size_t, _P, C.c_uint32]),
    ("fskhip_xmodem_snapshot_info_get", C.c_int, [_P, C.c_size_t, C.POINTER(XModemSnapshotInfo)]),
    ("fskhip_xmodem_rx_remap", C.c_int, [_P, _P, _P, C.c_uint32]),
    ("fskhip_xmodem_rx_snapshot_bytes", C.c_size_t, [_P, _P, C.c_uint32]),
    ("fskhip_xmodem_rx_snapshot", C.c_int, [_P, _P, C.c_uint32, _P, C.c_size_t, C.POINTER(C.c_size_t)]),
    ("fskhip_xmodem_rx_restore", C.c_int, [_P, _P, C.c_size_t, _P, C.c_uint32]),
    ("fskhip_xmodem_tx_remap", C.c_int, [_P, _P, _P, C.c_uint32]),
    ("fskhip_xmodem_tx_snapshot_bytes", C.c_size_t, [_P, _P, C.c_uint32]),
    ("fskhip_xmodem_tx_snapshot", C.c_int, [_P, _P, C.c_uint32, _P, C.c_size_t, C.POINTER(C.c_size_t)]),
    ("fskhip_xmodem_tx_restore", C.c_int, [_P, _P, C.c_size_t, _P, C.c_uint32]),
    ("fskhip_xmodem_recv_remap", C.c_int, [_P, _P, _P, C.c_uint32]),
    ("fskhip_xmodem_recv_snapshot_bytes", C.c_size_t, [_P, _P, C.c_uint32]),
    ("fskhip_xmodem_recv_snapshot", C.c_int, [_P, _P, C.c_uint32, _P, C.c_size_t, C.POINTER(C.c_size_t)]),
    ("fskhip_xmodem_recv_restore", C.c_int, [_P, _P, C.c_size_t, _P, C.c_uint32]),
    ("fskhip_sinc_lowpass", C.c_int, [C.c_double, C.c_double, C.c_uint32, _P]),
    ("fskhip_sinc_highpass", C.c_int, [C.c_double, C.c_double, C.c_uint32, _P]),
    ("fskhip_sinc_bandpass", C.c_int, [C.c_double, C.c_double, C.c_double, C.c_uint32, _P]),
    ("fskhip_fir_create", C.c_int, [C.c_int, _P, C.c_uint32, C.c_uint32, C.c_int, C.POINTER(_P)]),
    ("fskhip_fir_destroy", C.c_int, [_P]),
    ("fskhip_fir_streams", C.c_uint32, [_P]),
    ("fskhip_iir_streams", C.c_uint32, [_P]),
    ("fskhip_fir_process_device", C.c_int, [_P, _P, C.c_size_t, C.c_size_t, _P, C.c_size_t, _P]),
    ("fskhip_fir_process_host", C.c_int, [_P, _P, C.c_size_t, C.c_size_t, _P, C.c_size_t]),
    ("fskhip_fir_reset", C.c_int, [_P, C.c_int64]),
    ("fskhip_resampler_create", C.c_int, [C.c_int, C.c_int, C.c_uint32, _P, C.c_uint32, C.c_uint32, C.c_int, C.POINTER(_P)]),
    ("fskhip_resampler_destroy", C.c_int, [_P]),
    ("fskhip_resampler_streams", C.c_uint32, [_P]),
    ("fskhip_resampler_history", C.c_uint32, [_P]),
    ("fskhip_resampler_reset", C.c_int, [_P, C.c_int64]),
    ("fskhip_resampler_up_device", C.c_int, [_P, _P, C.c_int, C.c_int, C.c_size_t, C.c_size_t, _P, C.c_size_t, _P]),
    ("fskhip_resampler_down_device", C.c_int, [_P, _P, C.c_size_t, C.c_size_t, _P, _P, C.c_int, C.c_int, C.c_size_t, _P]),
    ("fskhip_resampler_up_host", C.c_int, [_P, _P, C.c_int, C.c_int, C.c_size_t, C.c_size_t, _P, C.c_size_t]),
    ("fskhip_resampler_down_host", C.c_int, [_P, _P, C.c_size_t, C.c_size_t, _P, _P, C.c_int, C.c_int, C.c_size_t]),
    ("fskhip_resampler_state_get", C.c_int, [_P, _P]),
    ("fskhip_resampler_state_set", C.c_int, [_P, _P]),
    ("fskhip_resampler_remap", C.c_int, [_P, _P, C.c_uint32, C.POINTER(_P)]),
    ("fskhip_resampler_snapshot_bytes", C.c_int, [_P, C.c_uint32, C.POINTER(C.c_size_t)]),
    ("fskhip_resampler_snapshot", C.c_int, [_P, _P, C.c_uint32, _P, C.c_size_t, C.POINTER(C.c_size_t)]),
    ("fskhip_resampler_restore", C.c_int, [C.c_int, _P, C.c_size_t, _P, C.c_uint32, C.POINTER(_P)]),
    ("fskhip_resampler_snapshot_info_get", C.c_int, [_P, C.c_size_t, C.POINTER(ResamplerSnapshotInfo)]),
    ("fskhip_processor_process_rate_device", C.c_int, [_P, _P, _P, _P, C.c_int, C.c_int, C.c_size_t, C.c_size_t, _P, C.c_int, C.c_int, C.c_size_t, C.c_size_t, C.c_uint32, _P]),
    ("fskhip_processor_process_rate_host", C.c_int, [_P, _P, _P, _P, C.c_int, C.c_int, C.c_size_t, C.c_size_t, _P, C.c_int, C.c_int, C.c_size_t, C.c_size_t, C.c_uint32]),
    ("fskhip_ratecvt_create", C.c_int, [C.c_int, C.c_int, C.c_uint32, C.c_uint32, _P, C.c_uint32, C.c_uint32, C.c_int, C.POINTER(_P)]),
    ("fskhip_ratecvt_destroy", C.c_int, [_P]),
    ("fskhip_ratecvt_streams", C.c_uint32, [_P]),
    ("fskhip_ratecvt_history", C.c_uint32, [_P]),
    ("fskhip_ratecvt_reset", C.c_int, [_P, C.c_int64]),
    ("fskhip_ratecvt_capture_device", C.c_int, [_P, _P, C.c_int, C.c_int, C.c_size_t, C.c_size_t, _P, C.c_size_t, _P]),
    ("fskhip_ratecvt_playback_device", C.c_int, [_P, _P, C.c_size_t, C.c_size_t, _P, _P, C.c_int, C.c_int, C.c_size_t, _P]),
    ("fskhip_ratecvt_capture_host", C.c_int, [_P, _P, C.c_int, C.c_int, C.c_size_t, C.c_size_t, _P, C.c_size_t]),
    ("fskhip_ratecvt_playback_host", C.c_int, [_P, _P, C.c_size_t, C.c_size_t, _P, _P, C.c_int, C.c_int, C.c_size_t]),
    ("fskhip_ratecvt_state_get", C.c_int, [_P, _P]),
    ("fskhip_ratecvt_state_set", C.c_int, [_P, _P]),
    ("fskhip_processor_process_ratecvt_device", C.c_int, [_P, _P, _P, _P, C.c_int, C.c_int, C.c_size_t, C.c_size_t, _P, C.c_int, C.c_int, C.c_size_t, C.c_size_t, C.c_uint32, _P]),
    ("fskhip_processor_process_ratecvt_host", C.c_int, [_P, _P, _P, _P, C.c_int, C.c_int, C.c_size_t, C.c_size_t, _P, C.c_int, C.c_int, C.c_size_t, C.c_size_t, C.c_uint32]),
    ("fskhip_ratecvt_capture_any_device", C.c_int, [_P, _P, C.c_int, C.c_int, C.c_size_t, C.c_size_t, _P, C.c_size_t, _P, _P]),
    ("fskhip_ratecvt_playback_any_device", C.c_int, [_P, _P, C.c_size_t, C.c_size_t, _P, _P, C.c_int, C.c_int, C.c_size_t, _P, _P]),
    ("fskhip_ratecvt_capture_any_host", C.c_int, [_P, _P, C.c_int, C.c_int, C.c_size_t, C.c_size_t, _P, C.c_size_t, _P]),
    ("fskhip_ratecvt_playback_any_host", C.c_int, [_P, _P, C.c_size_t, C.c_size_t, _P, _P, C.c_int, C.c_int, C.c_size_t, _P]),
    ("fskhip_ratecvt_position", C.c_uint32, [_P]),
    ("fskhip_ratecvt_position_set", C.c_int, [_P, C.c_uint32]),
    ("fskhip_ratecvt_out_count_any", C.c_size_t, [_P, C.c_size_t]),
    ("fskhip_ratecvt_in_count_any", C.c_size_t, [_P, C.c_size_t]),
    ("fskhip_processor_process_ratecvt_any_device", C.c_int, [_P, _P, _P, _P, C.c_int, C.c_int, C.c_size_t, C.c_size_t, _P, C.c_int, C.c_int, C.c_size_t, C.c_size_t, C.c_uint32, _P]),
    ("fskhip_processor_process_ratecvt_any_host", C.c_int, [_P, _P, _P, _P, C.c_int, C.c_int, C.c_size_t, C.c_size_t, _P, C.c_int, C.c_int, C.c_size_t, C.c_size_t, C.c_uint32]),
    ("fskhip_ratecvt_remap", C.c_int, [_P, _P, C.c_uint32, C.POINTER(_P)]),
    ("fskhip_ratecvt_snapshot_bytes", C.c_int, [_P, C.c_uint32, C.POINTER(C.c_size_t)]),
    ("fskhip_ratecvt_snapshot", C.c_int, [_P, _P, C.c_uint32, _P, C.c_size_t, C.POINTER(C.c_size_t)]),
    ("fskhip_ratecvt_restore", C.c_int, [C.c_int, _P, C.c_size_t, _P, C.c_uint32, C.POINTER(_P)]),
    ("fskhip_ratecvt_snapshot_info_get", C.c_int, [_P, C.c_size_t, C.POINTER(RatecvtSnapshotInfo)]),
    ("fskhip_iir_create", C.c_int, [C.c_int, _P, C.c_uint32, _P, C.c_uint32, C.c_uint32, C.c_int, C.POINTER(_P)]),
    ("fskhip_iir_destroy", C.c_int, [_P]),
    ("fskhip_iir_get_coefficients", C.c_int, [_P, _P, C.POINTER(C.c_uint32), _P, C.POINTER(C.c_uint32)]),
    ("fskhip_iir_process_device", C.c_int, [_P, _P, C.c_size_t, C.c_size_t, _P, C.c_size_t, _P]),
    ("fskhip_iir_process_host", C.c_int, [_P, _P, C.c_size_t, C.c_size_t, _P, C.c_size_t]),
    ("fskhip_iir_process_f64_device", C.c_int, [_P, _P, C.c_size_t, C.c_size_t, _P, C.c_size_t, _P]),
    ("fskhip_iir_process_f64_host", C.c_int, [_P, _P, C.c_size_t, C.c_size_t, _P, C.c_size_t]),
    ("fskhip_iir_reset", C.c_int, [_P, C.c_int64]),
]
SYMBOL_NAMES = [s[0] for s in _SYMBOLS]

_lib = None


class FskHipError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("fskhip error %d: %s" % (code, msg))
        self.code = code


def lib():
    """Load libfskhip.so; raises if the HIP extension has not been built (no fallback)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                "libfskhip.so not found at %s: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "or `make -C webaudio_modem_amd/csrc` (there is no CPU fallback)" % LIB_PATH)
        L = C.CDLL(LIB_PATH)
        for name, res, args in _SYMBOLS:
            fn = getattr(L, name)  # AttributeError if the library does not export it
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def check(rc):
    if rc != OK:
        raise FskHipError(rc, lib().fskhip_last_error().decode("utf-8", "replace"))
    return rc


def check_busy(rc, text=None):
    """check() for the calls that can find a stream busy ('modulate', sendData, receiveData): FSKHIP_E_BUSY, and no other code,
    is the reference's own throw -- a plain RuntimeError with `text` (None: the library's message).  Every other failure,
    FSKHIP_E_HANDOFF among them, is check()'s FskHipError with its code."""
    if rc == E_BUSY:
        raise RuntimeError(text if text is not None else lib().fskhip_last_error().decode("utf-8", "replace"))
    return check(rc)
