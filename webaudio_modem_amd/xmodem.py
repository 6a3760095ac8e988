"""CRC-16 and XModem packets above the C ABI (include/fskhip_next.h): the reference's `CRC16`
(src/utils/crc16.ts) and `XModemPacket` (src/transports/xmodem/packet.ts) with the same names, argument meaning
and error texts, plus the batch forms that actually feed a GPU and `scan_bursts`, the receive checks of
XModemTransport (src/transports/xmodem/xmodem.ts:233-320) applied to the bytes a demodulate call returned; and
`XModemReceiverBatch`, the same grammar resident on the device over the RX rings of an `FSKProcessorBatch`, and
`XModemSenderBatch`, `sendData()` for every stream of one: files, packets and the waits' grammar on the device, and
`XModemFileReceiverBatch`, `receiveData()` for every stream of one: grammar, ACK / NAK, retries and the file on the device; and
`XModemTimers`, the wait timers of those two in the engine's sample clock, on the device as well.
The three resident classes follow their streams through `remapped`, `snapshot` and `from_snapshot`, as the engine and the processor do.
Everything computes in libfskhip.so; there is no CPU path here.
"""
import ctypes as C

import numpy as np

from . import _lib
from .engine import _blob, _struct_dict
from ._lib import XModemTxEvent, XT_IDLE, XT_WAIT_NAK, XT_WAIT_ACK, XT_WAIT_FINAL_ACK, XT_PROGRESS, XT_DONE, XT_MAX_RETRIES, XT_ABORTED  # noqa: F401
from ._lib import XModemRecvEvent, XR_IDLE, XR_SEND_NAK, XR_WAIT_BLOCK, XR_SEND_ACK, XR_PROGRESS, XR_DONE, XR_MAX_RETRIES, XR_ABORTED, XR_FILE_FULL  # noqa: F401
from ._lib import XModemResult, XM_NEED_MORE, XM_EOT, XM_TRUNCATED, XM_INVALID_SEQUENCE, XM_INVALID_CRC, \
    XM_UNEXPECTED_SEQUENCE  # noqa: F401


class ControlType:  # types.ts:29-34
    SOH, ACK, NAK, EOT = 0x01, 0x06, 0x15, 0x04


PacketConstants = dict(SOH=0x01, HEADER_SIZE=4, CRC_SIZE=2, MIN_PACKET_SIZE=6, MAX_PACKET_SIZE=261,
                       MAX_PAYLOAD_SIZE=255, MAX_SEQUENCE=255, MIN_DATA_SEQUENCE=1)  # types.ts:62-75

STATUS_NAMES = {XM_NEED_MORE: "need_more", XM_EOT: "eot", XM_TRUNCATED: "truncated",
                XM_INVALID_SEQUENCE: "invalid_sequence", XM_INVALID_CRC: "invalid_crc",
                XM_UNEXPECTED_SEQUENCE: "unexpected_sequence"}
# what XModemTransport throws where a scan ends with that status (xmodem.ts:273, 290, 318)
STATUS_ERRORS = {XM_INVALID_SEQUENCE: "Invalid sequence number", XM_INVALID_CRC: "Invalid CRC",
                 XM_UNEXPECTED_SEQUENCE: "Unexpected sequence number"}


def _pack_rows(rows, min_pitch=4):
    """list of bytes-like -> (uint8 [n][pitch] array, uint32 lens)."""
    rows = [bytes(r) for r in rows]
    lens = np.array([len(r) for r in rows], dtype=np.uint32)
    pitch = max(min_pitch, (int(lens.max()) + 3) // 4 * 4 if len(rows) else min_pitch)
    slab = np.zeros((len(rows), pitch), dtype=np.uint8)
    for i, r in enumerate(rows):
        slab[i, :len(r)] = np.frombuffer(r, dtype=np.uint8)
    return slab, lens


def crc16_batch(rows, device=0):
    """CRC16.calculate of every row; rows is a list of bytes-like or (uint8 [n][pitch], lens)."""
    slab, lens = rows if isinstance(rows, tuple) else _pack_rows(rows)
    slab = np.ascontiguousarray(slab, dtype=np.uint8)
    lens = np.ascontiguousarray(lens, dtype=np.uint32)
    out = np.zeros(len(lens), dtype=np.uint16)
    _lib.check(_lib.lib().fskhip_crc16_host(device, slab.ctypes.data, slab.shape[1], lens.ctypes.data, len(lens),
                                            out.ctypes.data))
    return out


class CRC16:
    """crc16.ts: CRC-16-CCITT, polynomial 0x1021, initial value 0xFFFF, no final xor."""
    POLYNOMIAL, INITIAL_VALUE, FINAL_XOR = 0x1021, 0xFFFF, 0x0000

    @staticmethod
    def calculate(data, device=0):
        return int(crc16_batch([data], device)[0])

    @staticmethod
    def verify(data, expectedCrc, device=0):
        return CRC16.calculate(data, device) == expectedCrc


def serialize_batch(seqs, payloads, device=0):
    """XModemPacket.serialize(createData(seq, payload)) per row -> list of bytes."""
    rows = [bytes(p) for p in payloads]
    for seq, p in zip(seqs, rows):  # createData's throws, before anything is sent to the device
        if seq < 1 or seq > 255:
            raise ValueError("Invalid sequence: %d. Must be 1-255." % seq)
        if len(p) > 255:
            raise ValueError("Payload too large: %d. Max 255 bytes." % len(p))
    slab, lens = _pack_rows(rows)
    seqs = np.ascontiguousarray(seqs, dtype=np.uint32)
    out_pitch = int(lens.max()) + 6 if len(rows) else 6
    out = np.zeros((len(rows), out_pitch), dtype=np.uint8)
    out_lens = np.zeros(len(rows), dtype=np.uint32)
    _lib.check(_lib.lib().fskhip_xmodem_serialize_host(device, slab.ctypes.data, slab.shape[1], lens.ctypes.data,
                                                       seqs.ctypes.data, len(rows), out.ctypes.data, out_pitch,
                                                       out_lens.ctypes.data))
    return [out[i, :out_lens[i]].tobytes() for i in range(len(rows))]


class XModemPacket:
    """packet.ts:17-66, one packet at a time (a batch of one on the device)."""

    @staticmethod
    def createData(sequence, payload, device=0):
        payload = bytes(payload)
        wire = serialize_batch([sequence], [payload], device)[0]
        return {"soh": wire[0], "sequence": wire[1], "invSequence": wire[2], "length": wire[3],
                "payload": payload, "checksum": (wire[-2] << 8) | wire[-1], "_wire": wire}

    @staticmethod
    def serialize(packet):
        if "_wire" in packet and packet["_wire"][4:-2] == bytes(packet["payload"]):
            return packet["_wire"]
        return bytes([packet["soh"], packet["sequence"], packet["invSequence"], packet["length"]]) + \
            bytes(packet["payload"]) + bytes([(packet["checksum"] >> 8) & 0xFF, packet["checksum"] & 0xFF])

    @staticmethod
    def verify(packet, device=0):
        return CRC16.calculate(packet["payload"], device) == packet["checksum"]

    @staticmethod
    def serializeControl(controlType):
        return bytes([controlType])


def scan_bursts(bursts, expected, device=0, data_pitch=None):
    """The receive grammar over one recorded burst per stream.  bursts: list of bytes-like (or (slab, counts));
    expected: the starting expectedSequence per stream.  Returns a list of dicts: status (XM_*), status_name,
    error (the reference's exception text or None), expected_after, packets, dropped, consumed, err_seq, err_len,
    crc_rx, crc_calc, data (assembled payload bytes)."""
    slab, counts = bursts if isinstance(bursts, tuple) else _pack_rows(bursts)
    slab = np.ascontiguousarray(slab, dtype=np.uint8)
    counts = np.ascontiguousarray(counts, dtype=np.uint32)
    n = len(counts)
    exp = np.ascontiguousarray(np.broadcast_to(np.asarray(expected, dtype=np.uint32), (n,)))
    if data_pitch is None:
        data_pitch = max(4, slab.shape[1])
    data = np.zeros((n, data_pitch), dtype=np.uint8)
    res = (XModemResult * max(1, n))()
    _lib.check(_lib.lib().fskhip_xmodem_scan_host(device, slab.ctypes.data, slab.shape[1], counts.ctypes.data,
                                                  exp.ctypes.data, n, data.ctypes.data, data_pitch, res))
    out = []
    for i in range(n):
        r = res[i]
        d = {k: int(getattr(r, k)) for k, _ in XModemResult._fields_}
        d["status_name"] = STATUS_NAMES[d["status"]]
        d["error"] = STATUS_ERRORS.get(d["status"])
        d["data"] = data[i, :d["data_len"]].tobytes()
        out.append(d)
    return out


# fskhip_xmodem_result as a numpy record: the ten words, in order
RESULT_DTYPE = np.dtype([(k, "<u4" if t is C.c_uint32 else "<i4") for k, t in XModemResult._fields_])


XMODEM_SNAPSHOT_KINDS = {1: "rx", 2: "tx", 3: "recv"}


def xmodem_snapshot_info(snap):
    """fskhip_xmodem_snapshot_info_get: what an XModem snapshot holds -- kind (1 rx, 2 tx, 3 recv), n_streams, param0 / param1
    (tx: max_payload_size / max_retries; recv: file_capacity / max_retries), file_bytes -- validated on the host, no device needed"""
    b = _blob(snap)
    info = _lib.XModemSnapshotInfo()
    _lib.check(_lib.lib().fskhip_xmodem_snapshot_info_get(b.ctypes.data, b.nbytes, C.byref(info)))
    return _struct_dict(info)


class _Lifecycle:
    """remapped / snapshot / from_snapshot of the three resident classes (fskhip_xmodem_<_KIND>_remap, _snapshot_bytes, _snapshot,
    _restore): the handle's state follows its streams with the map the engine and the processor were carried with.  A class says
    how a new object like `self` is made over another processor (_like) and from an image's parameters (_from_info)."""
    _KIND = None

    def _fn(self, what):
        return getattr(self._L, "fskhip_xmodem_%s_%s" % (self._KIND, what))

    def remapped(self, processor, stream_map):
        """A new object over `processor` -- the destination the engine and the processor were remapped into with the same
        stream_map -- whose stream i continues stream stream_map[i] of this one, file included, or starts as a new transport
        where stream_map[i] is -1.  This object stays usable."""
        m = np.ascontiguousarray(stream_map, dtype=np.int64).reshape(-1)
        nxt = self._like(processor)
        try:
            _lib.check(self._fn("remap")(nxt._h, self._h, m.ctypes.data if len(m) else None, len(m)))
        except Exception:
            nxt.close()
            raise
        return nxt

    def snapshot(self, streams=None):
        """The image of streams `streams` (None: all, in order) as `bytes`: words and files.  This object is read only and stays usable."""
        sel = None if streams is None else np.ascontiguousarray(streams, dtype=np.int64).reshape(-1)
        n = self.n_streams if sel is None else len(sel)
        if sel is not None and not len(sel):
            sel = np.zeros(1, np.int64)   # (an empty selection, not "all": a non-null pointer with n = 0; `sel` keeps the array alive)
        sel_p = None if sel is None else sel.ctypes.data
        w = C.c_size_t(0)
        rc = self._fn("snapshot")(self._h, sel_p, n, None, 0, C.byref(w))   # the size
        if rc != _lib.E_OVERFLOW:
            _lib.check(rc)
        buf = np.zeros(max(w.value, 1), np.uint8)
        _lib.check(self._fn("snapshot")(self._h, sel_p, n, buf.ctypes.data, w.value, C.byref(w)))
        return buf[:w.value].tobytes()

    @classmethod
    def from_snapshot(cls, processor, snap, stream_map=None, **overrides):
        """A new object over `processor` that continues the records of a snapshot(): stream i continues record stream_map[i]
        (-1: a new transport; None: every record, in order).  The constructor's parameters are the image's unless overridden
        (file_capacity=, max_retries=)."""
        info = xmodem_snapshot_info(snap)
        if XMODEM_SNAPSHOT_KINDS.get(info["kind"]) != cls._KIND:
            raise ValueError("the snapshot is of kind %r, not %r" % (XMODEM_SNAPSHOT_KINDS.get(info["kind"]), cls._KIND))
        m = np.arange(info["n_streams"], dtype=np.int64) if stream_map is None else np.ascontiguousarray(stream_map, dtype=np.int64).reshape(-1)
        nxt = cls._from_info(processor, info, overrides)
        try:
            b = _blob(snap)
            _lib.check(nxt._fn("restore")(nxt._h, b.ctypes.data, b.nbytes, m.ctypes.data if len(m) else None, len(m)))
        except Exception:
            nxt.close()
            raise
        return nxt


class XModemReceiverBatch(_Lifecycle):
    """The receive side of XModemTransport for every stream of an FSKProcessorBatch, resident on the device
    (fskhip_xmodem_rx_*): a poll walks the RX rings in place, takes whole packets out of them and returns the accepted
    payloads and one result record per stream with something to answer -- an incomplete packet waits in its ring for
    the next poll.  expectedSequence and the running packetsReceived / packetsDropped live with this object.  Sending
    ACK / NAK, retries and timeouts are the caller's.  The processor must outlive it."""

    _KIND = "rx"

    def _like(self, processor):
        return XModemReceiverBatch(processor)

    @classmethod
    def _from_info(cls, processor, info, overrides):
        return cls(processor, **overrides)

    def __init__(self, processor):
        self.processor = processor
        self._L = _lib.lib()
        self.n_streams = processor.n_streams
        h = C.c_void_p()
        _lib.check(self._L.fskhip_xmodem_rx_create(processor._h, C.byref(h)))
        self._h = h
        self._cap_streams, self._cap_bytes = 0, 0

    def close(self):
        if getattr(self, "_h", None):
            self._L.fskhip_xmodem_rx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def poll(self, mask=None):
        """(streams, results, offsets, data): the streams with an event, ascending (uint32); their result records
        (RESULT_DTYPE); CSR offsets (uint32, len(streams) + 1); the accepted payload bytes (uint8) -- those of streams[i]
        are data[offsets[i]:offsets[i + 1]].  The lists are sized to the last poll's and grown on overflow: an
        overflowing call changes nothing and reports the true sizes."""
        m = None if mask is None else np.ascontiguousarray(np.asarray(mask).astype(bool), dtype=np.uint8)
        if m is not None and m.shape != (self.n_streams,):
            raise ValueError("mask must have one entry per stream")
        m_p = None if m is None else m.ctypes.data
        ne, nb = C.c_uint32(0), C.c_uint32(0)
        while True:
            cs, cb = self._cap_streams, self._cap_bytes
            streams, offsets = np.zeros(cs, np.uint32), np.zeros(cs + 1, np.uint32)
            results, data = np.zeros(cs, RESULT_DTYPE), np.zeros(cb, np.uint8)
            rc = self._L.fskhip_xmodem_rx_poll_host(self._h, m_p, streams.ctypes.data if cs else None, results.ctypes.data if cs else None,
                                                    offsets.ctypes.data if cs else None, cs, data.ctypes.data if cb else None, cb,
                                                    C.byref(ne), C.byref(nb))
            if rc != _lib.E_OVERFLOW:
                _lib.check(rc)
                break
            self._cap_streams, self._cap_bytes = max(cs, ne.value), max(cb, nb.value)
        n = ne.value
        return streams[:n], results[:n], offsets[:n + 1], data[:nb.value]

    def poll_active(self, mask=None):
        """{stream: (result dict, payload bytes)} of one poll; the dict has scan_bursts' keys"""
        streams, results, offsets, data = self.poll(mask)
        out = {}
        for i, s in enumerate(streams):
            d = {k: int(results[i][k]) for k in RESULT_DTYPE.names}
            d["status_name"] = STATUS_NAMES[d["status"]]
            d["error"] = STATUS_ERRORS.get(d["status"])
            out[int(s)] = (d, data[offsets[i]:offsets[i + 1]].tobytes())
        return out

    def reset(self, stream=-1):
        """initializeReceive() (xmodem.ts:221-225): expectedSequence = 1 for one stream, or all"""
        _lib.check(self._L.fskhip_xmodem_rx_reset(self._h, int(stream)))

    def state(self):
        """{"expected", "packets", "dropped"}: uint32 arrays, one entry per stream"""
        out = {k: np.zeros(self.n_streams, np.uint32) for k in ("expected", "packets", "dropped")}
        _lib.check(self._L.fskhip_xmodem_rx_state_get(self._h, out["expected"].ctypes.data, out["packets"].ctypes.data, out["dropped"].ctypes.data))
        return out

    def set_state(self, expected=None, packets=None, dropped=None):
        """what state() returned, or any part of it (expected: 1..255)"""
        arrs = []
        for a in (expected, packets, dropped):
            if a is not None:
                a = np.ascontiguousarray(a, dtype=np.uint32)
                if a.shape != (self.n_streams,):
                    raise ValueError("state arrays must have one entry per stream")
            arrs.append(a)
        _lib.check(self._L.fskhip_xmodem_rx_state_set(self._h, *[None if a is None else a.ctypes.data for a in arrs]))


# fskhip_xmodem_tx_event as a numpy record: the eight words, in order
TX_EVENT_DTYPE = np.dtype([(k, "<u4" if t is C.c_uint32 else "<i4") for k, t in XModemTxEvent._fields_])
TX_STATE_NAMES = {XT_IDLE: "IDLE", XT_WAIT_NAK: "SENDING_WAIT_NAK", XT_WAIT_ACK: "SENDING_WAIT_ACK", XT_WAIT_FINAL_ACK: "SENDING_WAIT_FINAL_ACK"}
TX_STATUS_NAMES = {XT_PROGRESS: "progress", XT_DONE: "done", XT_MAX_RETRIES: "max_retries", XT_ABORTED: "aborted"}
# what sendData() throws where a poll ends with that status (xmodem.ts:116, 618, 622); an abort in the first wait: TX_ERROR_FIRST_WAIT
TX_STATUS_ERRORS = {XT_MAX_RETRIES: "Timeout - max retries exceeded", XT_ABORTED: "Operation aborted"}
TX_ERROR_FIRST_WAIT = "Operation aborted at sendData"
TX_WORDS = ("state", "sequence", "fragment_index", "retries", "packets_sent", "retransmitted")


class XModemSenderBatch(_Lifecycle):
    """The send side of XModemTransport for every stream of an FSKProcessorBatch, resident on the device (fskhip_xmodem_tx_*):
    `send` hands each stream a file, a `poll` takes what each waiting stream's RX ring holds as one demodulate() reply, and where
    the control byte a wait is waiting for has arrived it builds the next packet (or the EOT) on the device and starts its
    modulation on the processor.  One poll is one reply, so what a poll finds depends on when it happens, as it does in the
    reference.  The timers are the caller's: a wait that has lasted too long is ended through `abort`.  The processor must
    outlive it."""

    _KIND = "tx"

    def _like(self, processor):
        return XModemSenderBatch(processor, max_payload_size=self.max_payload_size, max_retries=self.max_retries)

    @classmethod
    def _from_info(cls, processor, info, overrides):
        return cls(processor, **dict(dict(max_payload_size=info["param0"], max_retries=info["param1"]), **overrides))

    def __init__(self, processor, max_payload_size=128, max_retries=10):
        self.processor = processor
        self._L = _lib.lib()
        self.n_streams = processor.n_streams
        self.max_payload_size, self.max_retries = max_payload_size, max_retries
        h = C.c_void_p()
        _lib.check(self._L.fskhip_xmodem_tx_create(processor._h, max_payload_size, max_retries, C.byref(h)))
        self._h = h
        self._cap_streams = 0

    def close(self):
        if getattr(self, "_h", None):
            self._L.fskhip_xmodem_tx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _mask(self, mask, name="mask"):
        if mask is None:
            return None
        m = np.ascontiguousarray(np.asarray(mask).astype(bool), dtype=np.uint8)
        if m.shape != (self.n_streams,):
            raise ValueError("%s must have one entry per stream" % name)
        return m

    def send(self, files, mask=None):
        """sendData(files[s]) for every stream (or those of `mask`; the other entries are ignored and may be None): the files go to
        the device, the streams wait for the receiver's first NAK.  Nothing is transmitted yet.  A stream that is still sending
        raises RuntimeError with the reference's 'Transport busy' text, and nothing is started."""
        if len(files) != self.n_streams:
            raise ValueError("need one file per stream")
        m = self._mask(mask)
        rows = [bytes(f) if (m is None or m[s]) and f is not None else b"" for s, f in enumerate(files)]
        offsets = np.zeros(self.n_streams + 1, np.uint64)
        offsets[1:] = np.cumsum([len(r) for r in rows], dtype=np.uint64)
        data = np.frombuffer(b"".join(rows), np.uint8)
        rc = self._L.fskhip_xmodem_tx_send_host(self._h, None if m is None else m.ctypes.data, offsets.ctypes.data, data.ctypes.data if len(data) else None)
        _lib.check_busy(rc)

    def poll(self, mask=None, abort=None):
        """(streams, events): the streams where something happened, ascending (uint32), and their event records
        (TX_EVENT_DTYPE).  abort: the streams whose wait has timed out.  The lists are sized to the last poll's and grown on
        overflow: an overflowing call changes nothing and reports the true count."""
        m, a = self._mask(mask), self._mask(abort, "abort")
        ne = C.c_uint32(0)
        while True:
            cs = self._cap_streams
            streams, events = np.zeros(cs, np.uint32), np.zeros(cs, TX_EVENT_DTYPE)
            rc = self._L.fskhip_xmodem_tx_poll_host(self._h, None if m is None else m.ctypes.data, None if a is None else a.ctypes.data,
                                                    streams.ctypes.data if cs else None, events.ctypes.data if cs else None, cs, C.byref(ne))
            if rc != _lib.E_OVERFLOW:
                _lib.check(rc)
                break
            self._cap_streams = max(cs, ne.value)
        return streams[:ne.value], events[:ne.value]

    def poll_active(self, mask=None, abort=None):
        """{stream: event dict} of one poll; the dict has the record's words plus status_name, state_name and error (the text
        sendData() would have thrown, or None)"""
        streams, events = self.poll(mask, abort)
        out = {}
        for s, e in zip(streams, events):
            d = {k: int(e[k]) for k in TX_EVENT_DTYPE.names}
            d["status_name"], d["state_name"] = TX_STATUS_NAMES[d["status"]], TX_STATE_NAMES[d["state_after"]]
            d["error"] = TX_STATUS_ERRORS.get(d["status"])
            out[int(s)] = d
        return out

    def reset(self, stream=-1):
        """reset() (xmodem.ts:370-383) for one stream, or all: IDLE, sequence 1, the file dropped, the counters 0"""
        _lib.check(self._L.fskhip_xmodem_tx_reset(self._h, int(stream)))

    def state(self):
        """{"state", "sequence", "fragment_index", "retries", "packets_sent", "retransmitted"}: uint32 arrays, one entry per stream"""
        out = {k: np.zeros(self.n_streams, np.uint32) for k in TX_WORDS}
        _lib.check(self._L.fskhip_xmodem_tx_state_get(self._h, *[out[k].ctypes.data for k in TX_WORDS]))
        return out

    def set_state(self, **words):
        """what state() returned, or any part of it, after send() on this handle (validated as a whole before anything is set)"""
        arrs = []
        for k in TX_WORDS:
            a = words.pop(k, None)
            if a is not None:
                a = np.ascontiguousarray(a, dtype=np.uint32)
                if a.shape != (self.n_streams,):
                    raise ValueError("state arrays must have one entry per stream")
            arrs.append(a)
        if words:
            raise TypeError("unknown state words: %s" % ", ".join(sorted(words)))
        _lib.check(self._L.fskhip_xmodem_tx_state_set(self._h, *[None if a is None else a.ctypes.data for a in arrs]))


# fskhip_xmodem_recv_event as a numpy record: the twelve words, in order
RECV_EVENT_DTYPE = np.dtype([(k, "<u4" if t is C.c_uint32 else "<i4") for k, t in XModemRecvEvent._fields_])
RECV_STATE_NAMES = {XR_IDLE: "IDLE", XR_SEND_NAK: "RECEIVING_SEND_NAK", XR_WAIT_BLOCK: "RECEIVING_WAIT_BLOCK", XR_SEND_ACK: "RECEIVING_SEND_ACK"}
RECV_STATUS_NAMES = {XR_PROGRESS: "progress", XR_DONE: "done", XR_MAX_RETRIES: "max_retries", XR_ABORTED: "aborted", XR_FILE_FULL: "file_full"}
# what receiveData() throws where a poll ends with that status (xmodem.ts:235, 256); FILE_FULL is the resident store's own limit
RECV_STATUS_ERRORS = {XR_MAX_RETRIES: "Receive failed after max retries", XR_ABORTED: "Operation aborted", XR_FILE_FULL: "File store full"}
RECV_WORDS = ("state", "expected", "retries", "file_len", "packets_received", "dropped", "packets_sent")


class XModemFileReceiverBatch(_Lifecycle):
    """receiveData() of XModemTransport for every stream of an FSKProcessorBatch, resident on the device (fskhip_xmodem_recv_*):
    `start` sends the initial NAK, a `poll` walks each waiting stream's RX ring up to the first step of the receive grammar that
    owes a reply, appends an accepted payload to the stream's file on the device, counts retries and starts the ACK or NAK on the
    processor.  Only events come back; `files` reads the assembled files once, at the end.  The timers are the caller's: a wait
    that has lasted too long is named in `timeout`, an external abort in `abort`.  The processor must outlive it."""

    _KIND = "recv"

    def _like(self, processor):
        return XModemFileReceiverBatch(processor, file_capacity=self.file_capacity, max_retries=self.max_retries)

    @classmethod
    def _from_info(cls, processor, info, overrides):
        return cls(processor, **dict(dict(file_capacity=info["param0"], max_retries=info["param1"]), **overrides))

    def __init__(self, processor, file_capacity=65536, max_retries=10):
        self.processor = processor
        self._L = _lib.lib()
        self.n_streams = processor.n_streams
        self.file_capacity, self.max_retries = file_capacity, max_retries
        h = C.c_void_p()
        _lib.check(self._L.fskhip_xmodem_recv_create(processor._h, file_capacity, max_retries, C.byref(h)))
        self._h = h
        self._cap_streams = 0

    def close(self):
        if getattr(self, "_h", None):
            self._L.fskhip_xmodem_recv_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _mask(self, mask, name="mask"):
        if mask is None:
            return None
        m = np.ascontiguousarray(np.asarray(mask).astype(bool), dtype=np.uint8)
        if m.shape != (self.n_streams,):
            raise ValueError("%s must have one entry per stream" % name)
        return m

    def _sel(self, streams):
        sel = np.arange(self.n_streams, dtype=np.uint32) if streams is None else np.ascontiguousarray(streams, dtype=np.uint32)
        if sel.ndim != 1:
            raise ValueError("streams must be a list of stream indices")
        return sel

    def start(self, mask=None):
        """receiveData() up to its first wait for every stream (or those of `mask`): expected 1, an empty file, retries 0, and the
        initial NAK is modulated.  A stream that is still receiving, or whose processor is mid-modulation, raises RuntimeError
        with the reference's text, and nothing is started."""
        m = self._mask(mask)
        rc = self._L.fskhip_xmodem_recv_start_host(self._h, None if m is None else m.ctypes.data)
        _lib.check_busy(rc)

    def poll(self, mask=None, timeout=None, abort=None):
        """(streams, events): the streams where something happened, ascending (uint32), and their event records
        (RECV_EVENT_DTYPE).  timeout: the streams whose wait's timer has fired; abort: the streams to abort.  The lists are sized
        to the last poll's and grown on overflow: an overflowing call changes nothing and reports the true count."""
        m, t, a = self._mask(mask), self._mask(timeout, "timeout"), self._mask(abort, "abort")
        ne = C.c_uint32(0)
        while True:
            cs = self._cap_streams
            streams, events = np.zeros(cs, np.uint32), np.zeros(cs, RECV_EVENT_DTYPE)
            rc = self._L.fskhip_xmodem_recv_poll_host(self._h, *[None if x is None else x.ctypes.data for x in (m, t, a)],
                                                      streams.ctypes.data if cs else None, events.ctypes.data if cs else None, cs, C.byref(ne))
            if rc != _lib.E_OVERFLOW:
                _lib.check(rc)
                break
            self._cap_streams = max(cs, ne.value)
        return streams[:ne.value], events[:ne.value]

    def poll_active(self, mask=None, timeout=None, abort=None):
        """{stream: event dict} of one poll; the dict has the record's words plus status_name, state_name and error (the text
        receiveData() would have thrown, or None)"""
        streams, events = self.poll(mask, timeout, abort)
        out = {}
        for s, e in zip(streams, events):
            d = {k: int(e[k]) for k in RECV_EVENT_DTYPE.names}
            d["status_name"], d["state_name"] = RECV_STATUS_NAMES[d["status"]], RECV_STATE_NAMES[d["state_after"]]
            d["error"] = RECV_STATUS_ERRORS.get(d["status"])
            out[int(s)] = d
        return out

    def files(self, streams=None):
        """the assembled files of `streams` (default: all), a list of bytes: packed on the device, one copy"""
        sel = self._sel(streams)
        offsets, nb = np.zeros(len(sel) + 1, np.uint64), C.c_uint64(0)
        sel_p = sel.ctypes.data if len(sel) else None
        rc = self._L.fskhip_xmodem_recv_files_host(self._h, sel_p, len(sel), offsets.ctypes.data, None, 0, C.byref(nb))   # the size
        if rc != _lib.E_OVERFLOW:
            _lib.check(rc)
        data = np.zeros(nb.value, np.uint8)
        if nb.value:
            _lib.check(self._L.fskhip_xmodem_recv_files_host(self._h, sel_p, len(sel), offsets.ctypes.data, data.ctypes.data, data.nbytes, C.byref(nb)))
        return [data[int(offsets[i]):int(offsets[i + 1])].tobytes() for i in range(len(sel))]

    def set_files(self, files, mask=None):
        """puts files back (one per stream; those of `mask`, the other entries are ignored and may be None): before set_state, to
        carry a receiver across a remap or a restore"""
        if len(files) != self.n_streams:
            raise ValueError("need one file per stream")
        m = self._mask(mask)
        sel = np.array([s for s in range(self.n_streams) if m is None or m[s]], np.uint32)
        rows = [bytes(files[s]) for s in sel]
        offsets = np.zeros(len(sel) + 1, np.uint64)
        offsets[1:] = np.cumsum([len(r) for r in rows], dtype=np.uint64)
        data = np.frombuffer(b"".join(rows), np.uint8)
        _lib.check(self._L.fskhip_xmodem_recv_files_set_host(self._h, sel.ctypes.data if len(sel) else None, len(sel), offsets.ctypes.data,
                                                             data.ctypes.data if len(data) else None))

    def reset(self, stream=-1):
        """reset() (xmodem.ts:370-383) for one stream, or all: IDLE, expected 1, retries 0, an empty file, the counters 0"""
        _lib.check(self._L.fskhip_xmodem_recv_reset(self._h, int(stream)))

    def state(self):
        """{"state", "expected", "retries", "file_len", "packets_received", "dropped", "packets_sent"}: uint32 arrays, one entry per stream"""
        out = {k: np.zeros(self.n_streams, np.uint32) for k in RECV_WORDS}
        _lib.check(self._L.fskhip_xmodem_recv_state_get(self._h, *[out[k].ctypes.data for k in RECV_WORDS]))
        return out

    def set_state(self, **words):
        """what state() returned, or any part of it (validated as a whole before anything is set)"""
        arrs = []
        for k in RECV_WORDS:
            a = words.pop(k, None)
            if a is not None:
                a = np.ascontiguousarray(a, dtype=np.uint32)
                if a.shape != (self.n_streams,):
                    raise ValueError("state arrays must have one entry per stream")
            arrs.append(a)
        if words:
            raise TypeError("unknown state words: %s" % ", ".join(sorted(words)))
        _lib.check(self._L.fskhip_xmodem_recv_state_set(self._h, *[None if a is None else a.ctypes.data for a in arrs]))


TIMER_WORDS = ("waited", "mark")
TIMER_WAS_PENDING = 4   # mark: bits 0-1 the stage the timer was armed for (0..2, a sender's is always 0), bit 2 was-pending


def xmodem_timer_snapshot_info(snap):
    """fskhip_xmodem_timer_snapshot_info_get: what an XModemTimers snapshot holds -- kind (2 tx, 3 recv), n_streams,
    timeout_samples -- validated on the host, no device needed"""
    b = _blob(snap)
    info = _lib.XModemTimerSnapshotInfo()
    _lib.check(_lib.lib().fskhip_xmodem_timer_snapshot_info_get(b.ctypes.data, b.nbytes, C.byref(info)))
    return _struct_dict(info)


class XModemTimers(_Lifecycle):
    """The `timeoutMs` timers of sendData() / receiveData() for every stream of an XModemFileReceiverBatch or an XModemSenderBatch,
    resident on the device in the engine's sample clock (fskhip_xmodem_timer_*): `poll` is the handle's own poll between a fire
    and an arm pass, so a receiver's timeout mask and a sender's abort mask are built on the device and a lost packet is recovered
    from without the host reading any per-stream word.  `elapsed` is the engine samples processed since this object's previous
    poll.  The timers are quantised to the polls (a wait ends at the first poll at or after its deadline): poll once per quantum.
    The external abort stays the caller's (`abort`).  remapped / snapshot of the handle do not carry the timers; they follow
    their streams through remapped / snapshot / from_snapshot here, with the map the handle was carried with, so that a running
    wait goes on from where it was.  Close it before its handle."""

    _KIND = "timer"   # (_Lifecycle: fskhip_xmodem_timer_snapshot and its kin; snapshot() is _Lifecycle's as it is)

    def remapped(self, handle, stream_map, timeout_samples=None):
        """A new object over `handle` -- the receiver or sender this one's handle was remapped into with the same stream_map --
        whose stream i continues the wait of stream stream_map[i] of this one, or has a fresh timer where stream_map[i] is -1.
        The timeout is this object's unless given.  This object stays usable."""
        m = np.ascontiguousarray(stream_map, dtype=np.int64).reshape(-1)
        src = self._live()
        nxt = XModemTimers(handle, self.timeout_samples if timeout_samples is None else timeout_samples)
        try:
            _lib.check(self._L.fskhip_xmodem_timer_remap(nxt._h, src, m.ctypes.data if len(m) else None, len(m)))
        except Exception:
            nxt.close()
            raise
        return nxt

    @classmethod
    def from_snapshot(cls, handle, snap, stream_map=None, timeout_samples=None):
        """A new object over `handle` that continues the records of a snapshot(): stream i continues record stream_map[i]
        (-1: a fresh timer; None: every record, in order).  The timeout is the image's unless given."""
        info = xmodem_timer_snapshot_info(snap)
        m = np.arange(info["n_streams"], dtype=np.int64) if stream_map is None else np.ascontiguousarray(stream_map, dtype=np.int64).reshape(-1)
        nxt = cls(handle, info["timeout_samples"] if timeout_samples is None else timeout_samples)
        try:
            if XMODEM_SNAPSHOT_KINDS[info["kind"]] != nxt._kind:
                raise ValueError("the snapshot is of kind %r, the handle's is %r" % (XMODEM_SNAPSHOT_KINDS[info["kind"]], nxt._kind))
            b = _blob(snap)
            _lib.check(nxt._L.fskhip_xmodem_timer_restore(nxt._h, b.ctypes.data, b.nbytes, m.ctypes.data if len(m) else None, len(m)))
        except Exception:
            nxt.close()
            raise
        return nxt

    def __init__(self, handle, timeout_samples=144000):
        if isinstance(handle, XModemFileReceiverBatch):
            kind = "recv"
        elif isinstance(handle, XModemSenderBatch):
            kind = "tx"
        else:
            raise TypeError("XModemTimers needs an XModemFileReceiverBatch or an XModemSenderBatch")
        if not getattr(handle, "_h", None):
            raise ValueError("the handle has been closed")
        self.handle, self._kind = handle, kind
        self._L = _lib.lib()
        self.n_streams = handle.n_streams
        self.timeout_samples = int(timeout_samples)
        self._dtype = RECV_EVENT_DTYPE if kind == "recv" else TX_EVENT_DTYPE
        self._poll = getattr(self._L, "fskhip_xmodem_%s_poll_timed_host" % kind)
        h = C.c_void_p()
        _lib.check(getattr(self._L, "fskhip_xmodem_timer_create_" + kind)(handle._h, self.timeout_samples, C.byref(h)))
        self._h = h
        self._cap_streams = 0

    @classmethod
    def from_ms(cls, handle, timeout_ms, sample_rate=48000):
        """timeoutMs in the engine's clock: timeout_ms * sample_rate / 1000 samples, rounded up"""
        return cls(handle, timeout_samples=-(-int(timeout_ms) * int(sample_rate) // 1000))

    def close(self):
        if getattr(self, "_h", None):
            self._L.fskhip_xmodem_timer_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _live(self):
        if not getattr(self, "_h", None):
            raise ValueError("the timers have been closed")
        if not getattr(self.handle, "_h", None):
            raise ValueError("the timers' handle has been closed")
        return self._h

    def poll(self, elapsed, mask=None, abort=None):
        """(streams, events), exactly what the handle's own poll returns.  elapsed: engine samples since the previous poll; abort:
        the streams to abort from outside.  An overflowing call changes nothing, the timers included, and is repeated with
        larger lists."""
        h = self._live()
        if not 0 <= int(elapsed) <= 0xFFFFFFFF:
            raise ValueError("elapsed must fit 32 bits")
        m, a = self.handle._mask(mask), self.handle._mask(abort, "abort")
        ne = C.c_uint32(0)
        while True:
            cs = self._cap_streams
            streams, events = np.zeros(cs, np.uint32), np.zeros(cs, self._dtype)
            rc = self._poll(h, int(elapsed), None if m is None else m.ctypes.data, None if a is None else a.ctypes.data,
                            streams.ctypes.data if cs else None, events.ctypes.data if cs else None, cs, C.byref(ne))
            if rc != _lib.E_OVERFLOW:
                _lib.check(rc)
                break
            self._cap_streams = max(cs, ne.value)
        return streams[:ne.value], events[:ne.value]

    def poll_active(self, elapsed, mask=None, abort=None):
        """{stream: event dict} of one poll, as the handle's poll_active gives it"""
        streams, events = self.poll(elapsed, mask, abort)
        names = (RECV_STATUS_NAMES, RECV_STATE_NAMES, RECV_STATUS_ERRORS) if self._kind == "recv" else (TX_STATUS_NAMES, TX_STATE_NAMES, TX_STATUS_ERRORS)
        out = {}
        for s, e in zip(streams, events):
            d = {k: int(e[k]) for k in self._dtype.names}
            d["status_name"], d["state_name"] = names[0][d["status"]], names[1][d["state_after"]]
            d["error"] = names[2].get(d["status"])
            out[int(s)] = d
        return out

    def reset(self, stream=-1):
        """waited 0, mark 0 for one stream, or all"""
        _lib.check(self._L.fskhip_xmodem_timer_reset(self._live(), int(stream)))

    def state(self):
        """{"waited", "mark"}: uint32 arrays, one entry per stream"""
        out = {k: np.zeros(self.n_streams, np.uint32) for k in TIMER_WORDS}
        _lib.check(self._L.fskhip_xmodem_timer_state_get(self._live(), *[out[k].ctypes.data for k in TIMER_WORDS]))
        return out

    def set_state(self, waited=None, mark=None):
        """what state() returned, or either part of it (validated before anything is set)"""
        arrs = []
        for a in (waited, mark):
            if a is not None:
                a = np.ascontiguousarray(a, dtype=np.uint32)
                if a.shape != (self.n_streams,):
                    raise ValueError("state arrays must have one entry per stream")
            arrs.append(a)
        _lib.check(self._L.fskhip_xmodem_timer_state_set(self._live(), *[None if a is None else a.ctypes.data for a in arrs]))
