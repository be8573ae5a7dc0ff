"""Host side of the rANS stream kernels (`pcc_rans_*`) and of their container: what the entropy models, `geometry.py` and
`attributes.py` share.

A container is `u32 streams | streams x u32 words per stream | the streams' words`.  Its host rules live here and nowhere else:
  * capacity and workspace come from the library's three sizing functions (`Plan`);
  * the encoder wants the division-free entries, the decoder the compact blob, of the cdf it codes with (`Tables`);
  * the decoder reads whole 8-byte words and looks one word ahead, so PAD zero bytes follow a container in device memory, and
    containers that share a buffer start at multiples of PAD (`stage`, `upload_string`, `align8`).
`encode` / `estimate` / `decode` queue one kernel each on the current stream and read nothing back: where the byte count or
the status word lands, and when it is read, is the caller's design.
"""
import ctypes as C
import warnings
from functools import cached_property

import numpy as np
import torch

from . import lib as L

PAD = 8


def align8(v):
    return (int(v) + PAD - 1) // PAD * PAD


def segments_for(symbols, per_stream, most):
    """Streams of a vector of `symbols` cut every `per_stream`: at least one, at most `most`."""
    return max(1, min(-(-int(symbols) // max(1, int(per_stream))), most))


# ---- tables -------------------------------------------------------------------------------------------------------------
def _enc_entries(cdf, sizes):
    tab = np.zeros(cdf.shape[0] * cdf.shape[1] * 2, dtype=np.uint64)
    L.check(L.load().pcc_rans_build_enc_table(L.nptr(cdf), cdf.shape[0], cdf.shape[1], L.nptr(sizes), L.nptr(tab)),
            "pcc_rans_build_enc_table")
    return tab.view(np.int64)


def _dec_blob(cdf, sizes):
    lib = L.load()
    blob = np.zeros(lib.pcc_rans_dec_table_bytes(cdf.shape[0], L.nptr(sizes)), dtype=np.uint8)
    L.check(lib.pcc_rans_build_dec_table(L.nptr(cdf), cdf.shape[0], cdf.shape[1], L.nptr(sizes), L.nptr(blob)),
            "pcc_rans_build_dec_table")
    return blob


class Tables:
    """What a coder needs on one device: cdf [rows, stride], sizes [rows], offsets [rows] (int32 tensors), the encoder entries
    `enc` and the decoder blob `dec`.  `enc` / `dec` are the tensors given (tables derived on the device, or uploaded with
    their cdf) or else built from the three tensors when first asked for."""

    def __init__(self, cdf, sizes, offsets, enc=None, dec=None):
        self.cdf, self.sizes, self.offsets = cdf, sizes, offsets
        if enc is not None:
            self.enc = enc
        if dec is not None:
            self.dec = dec

    def host(self):
        """(cdf, sizes, offsets) as contiguous int32 arrays: what the host single-stream coder takes."""
        return tuple(np.ascontiguousarray(t.detach().cpu().numpy().astype(np.int32)) for t in (self.cdf, self.sizes, self.offsets))

    @cached_property
    def enc(self):
        cdf, sizes, _ = self.host()
        return torch.from_numpy(_enc_entries(cdf, sizes)).to(self.cdf.device)

    @cached_property
    def dec(self):
        cdf, sizes, _ = self.host()
        return torch.from_numpy(_dec_blob(cdf, sizes)).to(self.cdf.device)


_FIXED = {}


def fixed_tables(owner, dev, cdf, sizes, offsets, enc=False, dec=False):
    """Tables built on the host that never change, uploaded once per (owner, device).  cdf=None: sizes and offsets alone, for
    a coder whose cdf changes from call to call (`fresh_cdf_tables`, or a cdf derived on the device)."""
    key = (owner, str(dev))
    if key not in _FIXED:
        arrays = (cdf, sizes, offsets, _enc_entries(cdf, sizes) if enc else None, _dec_blob(cdf, sizes) if dec else None)
        _FIXED[key] = Tables(*(None if a is None else torch.from_numpy(a).to(dev) for a in arrays))
    return _FIXED[key]


def fresh_cdf_tables(owner, dev, cdf, sizes, offsets):
    """Encoder tables of a cdf the host has just derived, over the owner's resident sizes and offsets."""
    entries = _enc_entries(cdf, sizes)
    const = fixed_tables(owner, dev, None, sizes, offsets)
    return Tables(torch.from_numpy(cdf).to(dev), const.sizes, const.offsets, enc=torch.from_numpy(entries).to(dev))


# ---- streams ------------------------------------------------------------------------------------------------------------
class Plan:
    """The streams of an [n, channels] symbol matrix coded as `groups` channel groups x `segments` row segments, and the sizes
    the encoder needs for them.  The only caller of the library's sizing functions."""

    def __init__(self, n, channels, groups, segments):
        self.n, self.channels, self.groups, self.segments = n, channels, groups, segments
        self.streams = groups * segments
        self.per_stream = L.load().pcc_rans_stream_symbols(n, channels, groups, segments)

    @cached_property
    def capacity(self):
        """Upper bound of the container's bytes."""
        return L.load().pcc_rans_container_max_bytes(self.per_stream, self.streams)

    @cached_property
    def ws_bytes(self):
        return L.load().pcc_rans_streams_ws_bytes(self.per_stream, self.streams)


def _addr(x):
    """Device address of a tensor (None: NULL), or the address a caller computed itself (an offset into a shared blob)."""
    return x if isinstance(x, int) else L.ptr(x)


def estimate(tables, sym, idx, bits256):
    """Queue the payload estimate of sym [n, c] (table rows idx, None: row = channel): an int64 sum in 1/256 bit at `bits256`."""
    L.call("pcc_rans_estimate_bits", L.ptr(sym), L.ptr(idx), sym.shape[0], sym.shape[1], L.ptr(tables.cdf), tables.cdf.shape[1],
           L.ptr(tables.sizes), L.ptr(tables.offsets), _addr(bits256), L.stream())


def encode(tables, plan, sym, idx, out, nbytes):
    """Queue the encoder: the container goes to `out` (plan.capacity bytes), its int64 byte count to `nbytes`."""
    ws = L.workspace(plan.ws_bytes, tables.cdf.device)
    L.call("pcc_rans_encode_streams", _addr(sym), _addr(idx), plan.n, plan.channels, plan.groups, plan.segments, L.ptr(tables.cdf),
           tables.cdf.shape[1], L.ptr(tables.sizes), L.ptr(tables.offsets), L.ptr(tables.enc), _addr(out), _addr(nbytes),
           L.ptr(ws), ws.numel(), L.stream())


def decode(tables, data, nbytes, idx, n, channels, groups, segments, out, status, form=None):
    """Queue the decoder of the padded container of `nbytes` bytes at `data` into out [n, channels] int32; the int32 status
    word at `status` stays zero unless the container is malformed.  form: 1 = a lane, 2 = a wave per stream, 0 = the
    library's choice through the same entry point (`pcc_rans_decode_streams_form`); None: the plain entry point."""
    args = (_addr(data), nbytes, _addr(idx), n, channels, groups, segments, L.ptr(tables.cdf), tables.cdf.shape[1],
            L.ptr(tables.sizes), L.ptr(tables.offsets), L.ptr(tables.dec), tables.dec.numel(), _addr(out), _addr(status), L.stream())
    if form is None:
        L.call("pcc_rans_decode_streams", *args)
    else:
        L.call("pcc_rans_decode_streams_form", *args, form)


# ---- containers on their way to the decoder -----------------------------------------------------------------------------
def stage(data, spans):
    """(uint8 array, offsets): the containers data[begin:end] of `spans` in one host buffer for ONE upload, each at a multiple
    of PAD with at least PAD zero bytes behind it; never shorter than PAD."""
    offsets, at = [], 0
    for b0, b1 in spans:
        offsets.append(at)
        at += align8(b1 - b0 + PAD)
    buf = np.zeros(max(at, PAD), dtype=np.uint8)
    for o, (b0, b1) in zip(offsets, spans):
        buf[o:o + b1 - b0] = np.frombuffer(data, np.uint8, b1 - b0, b0)
    return buf, offsets


class UploadedString:
    """A coded string together with its (padded) copy in device memory; behaves like the bytes for the host-side parsing."""

    def __init__(self, data, device_buf):
        self.data, self.device_buf = data, device_buf
        self.groups = getattr(data, "groups", 0)

    def __len__(self):
        return len(self.data)

    def __getitem__(self, i):
        return self.data[i]


def upload_string(data, dev):
    """The container's bytes on the device, padded, as an `UploadedString` that the entropy models' `decompress_rows` takes in
    place of the bytes -- so that a caller can start the copy early, on another stream."""
    if isinstance(data, UploadedString):
        return data
    nb = len(data)
    buf = torch.empty(nb + PAD, dtype=torch.uint8, device=dev)
    if nb:
        with warnings.catch_warnings():          # (a read-only view of the bytes: no host-side copy before the upload)
            warnings.simplefilter("ignore")
            src = torch.frombuffer(data, dtype=torch.uint8)
        buf[:nb].copy_(src)
    buf[nb:].zero_()
    return UploadedString(data, buf)


# ---- the host single-stream coder (CompressAI's `BufferedRansEncoder` byte layout) ----------------------------------------
def pmf_to_quantized_cdf(pmf, precision=16):
    """CompressAI `pmf_to_quantized_cdf` (C++ op) -> libpcc_hip host function."""
    pmf = np.ascontiguousarray(np.asarray(pmf, dtype=np.float32))
    out = np.zeros(len(pmf) + 1, dtype=np.int32)
    L.check(L.load().pcc_pmf_to_quantized_cdf(L.nptr(pmf), len(pmf), precision, L.nptr(out)), "pcc_pmf_to_quantized_cdf")
    return out


def host_encode(tables, sym, idx):
    """Symbols sym with table rows idx (int32 arrays) under the host tables (cdf, sizes, offsets) -> bytes, one stream."""
    cdf, sizes, offs = tables
    lib = L.load()
    sym = np.ascontiguousarray(sym, np.int32)
    cap = lib.pcc_rans_max_bytes(len(sym))
    out = np.zeros(cap, np.uint8)
    nb = C.c_int64(0)
    L.check(lib.pcc_rans_encode_host(L.nptr(sym), L.nptr(idx), len(sym), L.nptr(cdf), cdf.shape[1], L.nptr(sizes), L.nptr(offs),
                                     L.nptr(out), cap, C.byref(nb)), "pcc_rans_encode_host")
    return out[:nb.value].tobytes()


def host_decode(tables, data, idx):
    cdf, sizes, offs = tables
    buf = np.frombuffer(data, np.uint8).copy()
    out = np.zeros(len(idx), np.int32)
    L.check(L.load().pcc_rans_decode_host(L.nptr(buf), len(buf), L.nptr(idx), len(idx), L.nptr(cdf), cdf.shape[1], L.nptr(sizes),
                                          L.nptr(offs), L.nptr(out)), "pcc_rans_decode_host")
    return out
