#!/usr/bin/env python3
"""lh_bam_append on one aligned batch by five paths: the host writer at zlib's default level, the host writer at level 1, the device writer (lh_bam_set_device: host
records, device compressor), the device writer with the records made on the device too (lh_bam_set_device_records), and that writer fed from the context's resident
result (lh_bam_append_resident: no download).  Then align -> files both ways: lh_align_resident + lh_result_download + lh_bam_append (device records) against
lh_align_resident + lh_bam_append_resident, two runs each.
Per path: lh_bam_timings' phases, pairs/s, compressed against uncompressed bytes; for the device paths lh_bgzf_timings too, for the last lh_bam_records_timings and the rate of
k_brec_write; the two device paths' files are compared byte for byte.  Then (unless `writer-only`) what the compressor costs an align loop that runs beside it:
lh_bgzf_compress in a loop on a second thread for the whole of the align loop's measurement.

usage: bam_device_probe.py [genome Mb = 100] [barcodes of 100 pairs = 5000] [host threads = 16] [writer-only] [families]
families: the reads lie on the copies of configs[4]'s repeat families (workload.config4_genome at the genome's scale): tens of candidates per read"""
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
families = "families" in sys.argv[4:]
if families:
    g = workload.config4_genome(lib, int(mb * 1e6), scale=mb / 3060.0, n_alt=4, alt_len=200000)
    pac, l_pac, ctg = g["pac"], g["l_pac"], g["contigs"]
    idx = lib.index_build_device(pac, l_pac, ctg)
    idx.set_alt(g["alt_flags"])
    r = lib.synth_reads(pac, l_pac, g["windows"], seed=7, n_barcodes=nbc, pairs_per_barcode=100)
else:
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
print("batch: %d pairs on a %.0f Mb genome%s, %d host threads; %.1f candidates per read" % (b.n_pairs, mb, " (reads on repeat families)" if families else "", threads, res.n_cand / res.n_reads))


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


def one(tag, level=None, z=None, records=False, resident=False):
    out = os.path.join(d, tag)
    os.makedirs(out)
    w = lib.bam_writer(out, names, lens, threads=threads)
    if level is not None:
        lib.L.lh_bam_set_level(w.h, level)
    if z is not None:
        w.set_device(z)
        w.set_device_records(records)
    t0 = time.time()
    if resident:   # (the context still holds the batch's result: nothing has been uploaded or aligned since)
        w.append_resident(ctx, b)
    else:
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
    return dict(append=ta, close=tc, records=x.value, join=y.value, write=t.value, comp=comp, unc=unc, zt=zt, rt=rt, sha=sha, resident=resident)


def show(tag, m):
    print("%-22s append %.3f s (records %.3f, join %.3f, compress+write %.3f), close %.3f s -> %.0f pairs/s; %d -> %d bytes, ratio %.3f"
          % (tag, m["append"], m["records"], m["join"], m["write"], m["close"], b.n_pairs / (m["append"] + m["close"]), m["unc"], m["comp"], m["comp"] / m["unc"]))
    if m["zt"]:
        print("%-22s lh_bgzf_timings of the append's call: upload %.3f s, kernel %.3f s, download %.3f s (device time, chunks overlap)"
              % ("", m["zt"]["upload_s"], m["zt"]["kernel_s"], m["zt"]["download_s"]))
    if m["rt"]:   # every record is written twice (bc_sorted and its bucket): k_brec_write stores 2 x the uncompressed record bytes
        print("%-22s lh_bam_records_timings: gather %.4f s (%s), upload %.4f s, plan kernels %.4f s, write kernel %.4f s = %.1f GB/s of BAM bytes stored"
              % ("", m["rt"]["gather_s"], "device" if m.get("resident") else "host", m["rt"]["upload_s"], m["rt"]["plan_s"], m["rt"]["encode_s"], m["unc"] / max(m["rt"]["encode_s"], 1e-9) / 1e9))


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
    ms = one("s%d" % rep, z=z, records=True, resident=True)
    show("device, resident:", ms)
    print("%-22s its files and the device paths' are %s" % ("", "EQUAL byte for byte" if md["sha"] == ms["sha"] else "DIFFERENT"))


def align_to_files(tag, resident):
    """one batch from the resident reads to the closed file set: the parent's path downloads the result (the library's own block, no numpy copies: what a C host
    pays) and appends it with device records; the new path appends from the context"""
    out = os.path.join(d, tag)
    os.makedirs(out)
    w = lib.bam_writer(out, names, lens, threads=threads)
    w.set_device(z)
    w.set_device_records(True)
    t0 = time.time()
    ctx.align_resident(opts)
    t1 = time.time()
    if resident:
        t2 = t1
        w.append_resident(ctx, b)
    else:
        p = C.POINTER(capi.LhResult)()
        lib.check(lib.L.lh_result_download(ctx.h, C.byref(p)))
        t2 = time.time()
        lib.check(lib.L.lh_bam_append(w.h, p, b.ptr))
        lib.L.lh_result_free(p)
    t3 = time.time()
    rt = w.timings()
    w.close()
    t4 = time.time()
    sha = digest(out)
    shutil.rmtree(out)
    print("%-34s align %.3f s, download %.3f s, append %.3f s, close %.3f s: %.3f s = %.0f pairs/s; after the align: %.3f s"
          % (tag + ":", t1 - t0, t2 - t1, t3 - t2, t4 - t3, t4 - t0, b.n_pairs / (t4 - t0), t4 - t1))
    print("%-34s lh_bam_records_timings: gather %.4f s (%s), upload %.4f s, plan kernels %.4f s, write kernel %.4f s"
          % ("", rt["gather_s"], "device" if resident else "host", rt["upload_s"], rt["plan_s"], rt["encode_s"]))
    return t4 - t0, t4 - t1, sha


opts = lib.opts()
ctx.upload(b)
align_to_files("warm download + append", False)
align_to_files("warm append_resident", True)
tot = {False: [], True: []}
for rep in range(2):
    for resident in (False, True):
        tot[resident].append(align_to_files(("align + append_resident %d" if resident else "align + download + append %d") % rep, resident))
assert len({x[2] for v in tot.values() for x in v}) == 1, "the two paths' files differ"
for k, what in ((0, "align -> files"), (1, "result -> files (after the align)")):
    old, new = [x[k] for x in tot[False]], [x[k] for x in tot[True]]
    print("%s: download + append %s s (spread %.1f %%), append_resident %s s: the means' ratio %.2f x; the files are EQUAL byte for byte"
          % (what, " / ".join("%.3f" % x for x in old), 100 * (max(old) - min(old)) / min(old), " / ".join("%.3f" % x for x in new), sum(old) / sum(new)))
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
