#!/usr/bin/env python3
"""Kernel time of the two LDS-table rANS decoders (form 1: one lane per stream, form 2: one wave per stream) over the stream
count, HIP-event timed, on Gaussian symbols of SYMBOLS per stream -- the table behind the dispatch threshold in
csrc/pcc_rans.hip (profiles/rans_wave_decode_crossover.txt).  The C entry points are called directly: the Python stream policy
stops at 4096 streams, the C interface at 65536.
usage: python tools/rans_decode_forms.py [streams ...]"""
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from unified_point_cloud_compression_amd import lib as L
from unified_point_cloud_compression_amd.compressai.entropy_models import GaussianConditional, get_scale_table

SYMBOLS = 1400
REPEATS = 7
dev = torch.device("cuda:0")
lib = L.load()
gc = GaussianConditional(None).to(dev)
gc.update_scale_table(get_scale_table(), force=True)
cdf, sizes, offs = (x.to(dev).contiguous() for x in (gc._quantized_cdf, gc._cdf_length, gc._offset))
tab, enc = gc._dec_table(dev), gc._enc_table(dev)
print(f"# {L.device_info()}  symbols per stream {SYMBOLS}, table rows idx 0..47 uniform, best of {REPEATS} launches (HIP events)")
print(f"{'streams':>8s} {'bits/sym':>9s} {'lane us':>10s} {'wave us':>10s} {'lane ns/sym':>12s} {'wave ns/sym':>12s} {'wave/lane':>10s}")
for ns in [int(a) for a in sys.argv[1:]] or [96, 1408, 4096, 16384, 65536]:
    c = 128 if ns % 128 == 0 else 32
    segs = ns // c
    assert segs * c == ns
    rows = segs * SYMBOLS
    g = torch.Generator(device=dev).manual_seed(ns)
    idx = torch.randint(0, 48, (rows, c), generator=g, device=dev, dtype=torch.int32)
    sym = torch.round(torch.randn((rows, c), generator=g, device=dev) * gc.scale_table.to(dev)[idx.long()]).to(torch.int32)
    per = lib.pcc_rans_stream_symbols(rows, c, c, segs)
    assert per == SYMBOLS
    out = torch.zeros(lib.pcc_rans_container_max_bytes(per, ns) + 8, dtype=torch.uint8, device=dev)
    nb = L.counter()
    ws = L.workspace(lib.pcc_rans_streams_ws_bytes(per, ns), dev)
    L.call("pcc_rans_encode_streams", L.ptr(sym), L.ptr(idx), rows, c, c, segs, L.ptr(cdf), cdf.shape[1], L.ptr(sizes),
           L.ptr(offs), L.ptr(enc), L.ptr(out), L.cptr(nb), L.ptr(ws), ws.numel(), L.stream())
    torch.cuda.synchronize()
    nbytes = int(L.read(nb)[0])
    out[nbytes:nbytes + 8].zero_()                        # the decoder looks up to two words ahead
    res, best = {}, {}
    for form in (1, 2):
        dec = torch.zeros_like(sym)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        times = []
        for _ in range(REPEATS + 1):                      # the first launch is the warm-up
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            L.call("pcc_rans_decode_streams_form", L.ptr(out), nbytes, L.ptr(idx), rows, c, c, segs, L.ptr(cdf), cdf.shape[1],
                   L.ptr(sizes), L.ptr(offs), L.ptr(tab), tab.numel(), L.ptr(dec), L.ptr(status), L.stream(), form)
            b.record()
            torch.cuda.synchronize()
            times.append(a.elapsed_time(b) * 1e3)
        assert int(status.item()) == 0 and torch.equal(dec, sym), f"form {form} at {ns} streams"
        best[form] = min(times[1:])
    print(f"{ns:8d} {nbytes * 8 / (rows * c):9.2f} {best[1]:10.1f} {best[2]:10.1f} {best[1] * 1e3 / SYMBOLS:12.1f} "
          f"{best[2] * 1e3 / SYMBOLS:12.1f} {best[2] / best[1]:10.2f}", flush=True)
    del idx, sym, out, dec
