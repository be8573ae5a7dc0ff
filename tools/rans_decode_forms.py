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
from unified_point_cloud_compression_amd import rans as R
from unified_point_cloud_compression_amd.compressai.entropy_models import GaussianConditional, get_scale_table

SYMBOLS = 1400
REPEATS = 7
dev = torch.device("cuda:0")
gc = GaussianConditional(None).to(dev)
gc.update_scale_table(get_scale_table(), force=True)
tabs = gc.tables(dev)
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
    plan = R.Plan(rows, c, c, segs)
    assert plan.per_stream == SYMBOLS
    out = torch.empty(plan.capacity, dtype=torch.uint8, device=dev)
    nb = L.counter()
    R.encode(tabs, plan, sym, idx, out, nb)
    nbytes = int(L.read(nb)[0])
    out = R.upload_string(out[:nbytes].cpu().numpy().tobytes(), dev).device_buf        # padded as the decoder wants it
    res, best = {}, {}
    for form in (1, 2):
        dec = torch.zeros_like(sym)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        times = []
        for _ in range(REPEATS + 1):                      # the first launch is the warm-up
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            R.decode(tabs, out, nbytes, idx, rows, c, c, segs, dec, status, form)
            b.record()
            torch.cuda.synchronize()
            times.append(a.elapsed_time(b) * 1e3)
        assert int(status.item()) == 0 and torch.equal(dec, sym), f"form {form} at {ns} streams"
        best[form] = min(times[1:])
    print(f"{ns:8d} {nbytes * 8 / (rows * c):9.2f} {best[1]:10.1f} {best[2]:10.1f} {best[1] * 1e3 / SYMBOLS:12.1f} "
          f"{best[2] * 1e3 / SYMBOLS:12.1f} {best[2] / best[1]:10.2f}", flush=True)
    del idx, sym, out, dec
