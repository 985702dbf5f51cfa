#!/usr/bin/env python3
"""lh_bam_append on one aligned batch by four paths: the host writer at zlib's default level, the host writer at level 1, the device writer (lh_bam_set_device: host
records, device compressor) and the device writer with the records made on the device too (lh_bam_set_device_records).
Per path: lh_bam_timings' phases, pairs/s, compressed against uncompressed bytes; for the device paths lh_bgzf_timings too, for the last lh_bam_records_timings and the rate of
k_brec_write; the two device paths' files are compared byte for byte.  Then (unless `writer-only`) what the compressor costs an align loop that runs beside it:
lh_bgzf_compress in a loop on a second thread for the whole of the align loop's measurement.

usage: bam_device_probe.py [genome Mb = 100] [barcodes of 100 pairs = 5000] [host threads = 16] [writer-only]"""
import ctypes as C
import hashlib
import os
import shutil
import struct
import sys
import tempfile
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from lariat_amd import capi, workload  # noqa: E402

lib = capi.load_library()
mb = float(sys.argv[1]) if len(sys.argv) > 1 else 100
nbc = int(sys.argv[2]) if len(sys.argv) > 2 else 5000
threads = int(sys.argv[3]) if len(sys.argv) > 3 else 16
ctg = workload.hg38_like_contigs(int(mb * 1e6))
l_pac = sum(c[1] for c in ctg)
pac = lib.synth_genome(l_pac, seed=workload.GENOME_SEED)
idx = lib.index_build_device(pac, l_pac, ctg)
r = lib.synth_reads(pac, l_pac, ctg, seed=7, n_barcodes=nbc, pairs_per_barcode=100)
base = "/dev/shm" if os.path.isdir("/dev/shm") else None
d = tempfile.mkdtemp(prefix="lh_bamdev_", dir=base)
fq = os.path.join(d, "c.fastq.gz")
lib.write_fastq9(fq, r, gz_level=1)
b = lib.ingest(fq, trim=7, max_pairs=nbc * 100).next(views_only=True)
ctx = idx.context(b.n_pairs)
res = ctx.align_barcodes(b)
cont = idx.contigs()
names, lens = [c[0] for c in cont], [c[1] for c in cont]
lib.L.lh_bam_timings.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double)]
print("batch: %d pairs on a %.0f Mb genome, %d host threads" % (b.n_pairs, mb, threads))


def sizes(out):
    """(compressed, uncompressed) bytes of a file set, from the members' BSIZE and ISIZE"""
    comp = unc = 0
    for f in os.listdir(out):
        raw = open(os.path.join(out, f), "rb").read()
        p = 0
        while p < len(raw):
            bsize = struct.unpack_from("<H", raw, p + 16)[0] + 1
            unc += struct.unpack_from("<I", raw, p + bsize - 4)[0]
            p += bsize
        comp += len(raw)
    return comp, unc


def digest(out):
    h = hashlib.sha256()
    for f in sorted(os.listdir(out)):
        h.update(f.encode())
        h.update(open(os.path.join(out, f), "rb").read())
    return h.hexdigest()


def one(tag, level=None, z=None, records=False):
    out = os.path.join(d, tag)
    os.makedirs(out)
    w = lib.bam_writer(out, names, lens, threads=threads)
    if level is not None:
        lib.L.lh_bam_set_level(w.h, level)
    if z is not None:
        w.set_device(z)
        w.set_device_records(records)
    t0 = time.time()
    w.append(res, b)
    ta = time.time() - t0
    x, y, t = C.c_double(), C.c_double(), C.c_double()
    lib.L.lh_bam_timings(w.h, C.byref(x), C.byref(y), C.byref(t))
    rt = w.timings() if records else None
    zt = z.timings() if z is not None else None
    t0 = time.time()
    w.close()
    tc = time.time() - t0
    comp, unc = sizes(out)
    sha = digest(out) if z is not None else None
    shutil.rmtree(out)
    return dict(append=ta, close=tc, records=x.value, join=y.value, write=t.value, comp=comp, unc=unc, zt=zt, rt=rt, sha=sha)


def show(tag, m):
    print("%-22s append %.3f s (records %.3f, join %.3f, compress+write %.3f), close %.3f s -> %.0f pairs/s; %d -> %d bytes, ratio %.3f"
          % (tag, m["append"], m["records"], m["join"], m["write"], m["close"], b.n_pairs / (m["append"] + m["close"]), m["unc"], m["comp"], m["comp"] / m["unc"]))
    if m["zt"]:
        print("%-22s lh_bgzf_timings of the append's call: upload %.3f s, kernel %.3f s, download %.3f s (device time, chunks overlap)"
              % ("", m["zt"]["upload_s"], m["zt"]["kernel_s"], m["zt"]["download_s"]))
    if m["rt"]:   # every record is written twice (bc_sorted and its bucket): k_brec_write stores 2 x the uncompressed record bytes
        print("%-22s lh_bam_records_timings: gather %.3f s (host), upload %.3f s, plan kernels %.3f s, write kernel %.3f s = %.1f GB/s of BAM bytes stored"
              % ("", m["rt"]["gather_s"], m["rt"]["upload_s"], m["rt"]["plan_s"], m["rt"]["encode_s"], m["unc"] / max(m["rt"]["encode_s"], 1e-9) / 1e9))


z = lib.bgzf()
one("warm", z=z)   # first use: page-locked staging is touched, the kernel's code is loaded
one("warmr", z=z, records=True)   # ... and the encoder's buffers are allocated
for rep in range(2):
    show("host, default level:", one("h%d" % rep))
    show("host, level 1:", one("l%d" % rep, level=1))
    md = one("d%d" % rep, z=z)
    show("device:", md)
    mr = one("r%d" % rep, z=z, records=True)
    show("device, records too:", mr)
    print("%-22s the two device paths' files are %s" % ("", "EQUAL byte for byte" if md["sha"] == mr["sha"] else "DIFFERENT"))
    print("%-22s append: %.3f s against %.3f s (%.2f x)" % ("", mr["append"], md["append"], md["append"] / mr["append"]))
if len(sys.argv) > 4 and sys.argv[4] == "writer-only":
    z.close()
    shutil.rmtree(d, ignore_errors=True)
    sys.exit(0)

# the align loop alone, then beside a thread that keeps the compressor busy: lh_bgzf_compress in a loop on the BAM bytes of this batch, so that k_bgzf and its
# transfers are in flight for the whole of the align loop's measurement (a writer thread would spend a third of its time encoding records on the host)
import gzip  # noqa: E402

out = os.path.join(d, "payload")
os.makedirs(out)
w = lib.bam_writer(out, names, lens, threads=threads)
lib.L.lh_bam_set_level(w.h, 1)
w.append(res, b)
w.close()
payload = gzip.decompress(open(os.path.join(out, "bc_sorted_bam.bam"), "rb").read())
shutil.rmtree(out)
ctx.upload(b)
opts = lib.opts()
N_ALIGN = 40


def align_rate(n):
    t0 = time.time()
    for _ in range(n):
        ctx.align_resident(opts)
        ctx.download()
    return n * b.n_pairs / (time.time() - t0)


def compress_rate(n):
    t0 = time.time()
    for _ in range(n):
        z.compress(payload)
    return n * len(payload) / (time.time() - t0)


align_rate(2)
compress_rate(1)
align_alone = align_rate(N_ALIGN)
comp_alone = compress_rate(3)
stop = threading.Event()
calls, busy = [0], [0.0]


def side():
    while not stop.is_set():
        t0 = time.time()
        z.compress(payload)
        busy[0] += time.time() - t0
        calls[0] += 1


th = threading.Thread(target=side)
th.start()
while calls[0] < 1:   # the compressor is running before the align loop starts ...
    time.sleep(0.01)
c0, b0, t0 = calls[0], busy[0], time.time()
align_beside = align_rate(N_ALIGN)
c1, b1, t1 = calls[0], busy[0], time.time()   # ... and still when it ends
stop.set()
th.join()
print("align loop, %d x %d pairs (resident batch, result downloaded): %.2f M pairs/s alone, %.2f M pairs/s beside lh_bgzf_compress in a loop (%.2f of the alone rate)"
      % (N_ALIGN, b.n_pairs, align_alone / 1e6, align_beside / 1e6, align_beside / align_alone))
print("lh_bgzf_compress of %d bytes: %.2f GB/s alone; beside the align loop %d calls finished in its %.2f s and the side thread was inside a call throughout (%.2f GB/s over the calls that finished)"
      % (len(payload), comp_alone / 1e9, c1 - c0, t1 - t0, (c1 - c0) * len(payload) / max(b1 - b0, 1e-9) / 1e9))
z.close()
shutil.rmtree(d, ignore_errors=True)
