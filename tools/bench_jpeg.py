"""Host JPEG decode (PIL) against the device route, on the GPU only (no GPU: an error, not a fallback); not part of bench.py.

  python tools/bench_jpeg.py [--frames 32] [--views 8] [--batch-frames 8] [--reps 10] [--subseq 0] [--wg-threads 0]

Setup: `frames` x `views` seeded 640x480 views (``inputs.synthetic_frame`` content plus texture noise, so the entropy stream is
of a realistic size), JPEG quality 90, 4:2:0, warped to 256x256 in calls of `batch-frames` frames.
Method: images/s of route A (PIL on one thread, then ``warp_views`` on the arrays) and route B (``warp_views`` on
``EncodedImage`` handles) with 1, 4 and 8 entropy-decode threads, in one session in the order A / B1 / B4 / B8 / A; each figure is
the median of `reps` passes over all views after one warm-up pass, with a device synchronise inside the timed window.
Also: the split of B into host entropy decode (wall clock), upload and the two kernels (HIP events; the colour kernel is the
difference between a whole reconstruct call and an IDCT-only one), the kernels' bytes moved per second against the HBM peak,
and the bytes uploaded per image on each route.
Route C is B with the Huffman decoding on the device too (``warp_views(jpeg_entropy="device")``; ``--subseq`` bytes per
subsequence, ``--wg-threads`` lanes per image, 0 = the library's defaults), measured in the same session as B8 / C / B8; its split:
host header parse + packing (wall clock), upload of the packed bytes, the entropy launch (memset + decode kernel + range-guard
kernel, HIP events; the decode kernel alone is the difference to a call whose range-guard kernel has nothing to do), the status
read-back, reconstruction; and the histogram of fixed-point rounds per image.  Prints one JSON line."""
import argparse
import ctypes
import io
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__  # noqa: E402,F401  (puts the package on the path)
import poem_v2_amd as pk  # noqa: E402
from poem_v2_amd import hip, transform, wds  # noqa: E402
from poem_v2_amd.jpeg import JpegDesc  # noqa: E402

HBM_PEAK_MEASURED = 6.29e12          # float4 copy on the MI355X (8.0e12 is the datasheet figure)


def make_views(frames, views, quality=90):
    from PIL import Image
    out = []
    for f in range(frames):
        rec = pk.inputs.synthetic_frame(f, n_cams=views, raw=(640, 480))
        rng = np.random.default_rng(1000 + f)
        for v in range(views):
            img = rec[f"image_{v}.png"].astype(np.int64)
            tex = rng.normal(0, 12, (60, 80, 3)).repeat(8, 0).repeat(8, 1) + rng.normal(0, 6, img.shape)     # coarse + fine texture
            buf = io.BytesIO()
            Image.fromarray(np.clip(img + tex, 0, 255).astype(np.uint8)).save(buf, format="JPEG", quality=quality, subsampling=2)
            out.append(buf.getvalue())
    return out


def median_rate(fn, n_images, reps):
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t)
    return n_images / statistics.median(times), min(times), max(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--views", type=int, default=8)
    ap.add_argument("--batch-frames", type=int, default=8)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--subseq", type=int, default=0)
    ap.add_argument("--wg-threads", type=int, default=0)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_jpeg.py measures the GPU route: it needs a GPU")
    dev = "cuda:0"
    streams = make_views(a.frames, a.views)
    n = len(streams)
    per = a.batch_frames * a.views
    eye = np.array([[256 / 640, 0, 0], [0, 256 / 480, 0]])
    batches = [streams[i:i + per] for i in range(0, n, per)]

    def route_a():
        for b in batches:
            transform.warp_views([wds.decode_rgb8(s) for s in b], [eye] * len(b), (256, 256), device=dev)

    def route_b():
        for b in batches:
            transform.warp_views([wds.EncodedImage(s) for s in b], [eye] * len(b), (256, 256), device=dev)

    res = {"images": n, "size": [480, 640], "quality": 90, "sampling": "4:2:0", "views_per_call": per, "reps": a.reps,
           "jpeg_bytes_per_image": sum(map(len, streams)) / n}
    res["A_host_images_per_s"] = median_rate(route_a, n, a.reps)[0]
    for t in (1, 4, 8):
        transform.set_jpeg_threads(t)
        transform.reset_jpeg_counts()
        res[f"B_device_threads{t}_images_per_s"] = median_rate(route_b, n, a.reps)[0]
        res[f"B_threads{t}_counts"] = transform.jpeg_counts()
    res["A_host_images_per_s_again"] = median_rate(route_a, n, a.reps)[0]

    # ---- route C: Huffman decoding on the device, between two runs of the 8-thread host route -------------------------------------
    def route_c():
        for b in batches:
            transform.warp_views([wds.EncodedImage(s) for s in b], [eye] * len(b), (256, 256), device=dev, jpeg_entropy="device")

    transform.set_jpeg_threads(8)
    transform.set_jpeg_entropy("host", subseq=a.subseq, wg_threads=a.wg_threads)
    res["B8_before_C_images_per_s"] = median_rate(route_b, n, a.reps)[0]
    transform.reset_jpeg_counts()
    res["C_device_entropy_images_per_s"] = median_rate(route_c, n, a.reps)[0]
    res["C_counts"] = transform.jpeg_counts()
    res["B8_after_C_images_per_s"] = median_rate(route_b, n, a.reps)[0]
    res["C_subseq"], res["C_wg_threads"] = a.subseq or 64, a.wg_threads or 1024

    # ---- the split of route B on one call's worth of views --------------------------------------------------------------------
    L = hip.lib()
    b = batches[0]
    m = len(b)
    bufs = [np.frombuffer(s, np.uint8) for s in b]
    ptrs = (ctypes.c_void_p * m)(*[x.ctypes.data for x in bufs])
    lens = (ctypes.c_int64 * m)(*[len(s) for s in b])
    descs, totals = (JpegDesc * m)(), (ctypes.c_int64 * 4)()
    hip.check(L.poem_jpeg_entropy_decode(ptrs, lens, m, descs, None, 0, totals, 1))
    need = int(totals[0])
    pinned = torch.empty(need, dtype=torch.uint8, pin_memory=True)
    for t in (1, 4, 8):
        ts = []
        for _ in range(a.reps + 1):
            t0 = time.perf_counter()
            hip.check(L.poem_jpeg_entropy_decode(ptrs, lens, m, descs, pinned.data_ptr(), need, totals, t))
            ts.append(time.perf_counter() - t0)
        res[f"entropy_decode_threads{t}_ms_per_image"] = statistics.median(ts[1:]) * 1e3 / m
    assert totals[3] == m, "a benchmark view was refused"
    blocks, quads = int(totals[1]), int(totals[2])
    ddev = torch.frombuffer(bytearray(bytes(descs)), dtype=torch.uint8).to(dev)
    cdev = torch.empty(need, dtype=torch.uint8, device=dev)
    offs = torch.arange(m, dtype=torch.int64, device=dev) * (480 * 640 * 3)
    out = torch.empty(m * 480 * 640 * 3, dtype=torch.uint8, device=dev)
    ws = torch.empty(L.poem_jpeg_workspace_bytes(blocks), dtype=torch.uint8, device=dev)

    def events(fn):
        fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
        return statistics.median(ms)

    def recon(q):
        hip.check(L.poem_jpeg_reconstruct(ddev.data_ptr(), cdev.data_ptr(), need, offs.data_ptr(), out.data_ptr(), out.numel(), m, blocks, q,
                                          ws.data_ptr(), ws.numel(), hip.stream()))

    up_ms = events(lambda: cdev.copy_(pinned, non_blocking=True))
    raw = torch.empty(m * 480 * 640 * 3, dtype=torch.uint8, pin_memory=True)
    up_raw_ms = events(lambda: out.copy_(raw, non_blocking=True))
    idct_ms = events(lambda: recon(0))
    both_ms = events(lambda: recon(quads))
    colour_ms = max(both_ms - idct_ms, 1e-6)
    idct_bytes, colour_bytes = need + 64 * blocks, 64 * blocks + m * 480 * 640 * 3
    res.update({"split_views": m, "upload_coef_ms_per_image": up_ms / m, "upload_pixels_ms_per_image": up_raw_ms / m,
                "idct_kernel_ms_per_image": idct_ms / m, "colour_kernel_ms_per_image": colour_ms / m,
                "idct_kernel_TB_per_s": idct_bytes / (idct_ms * 1e-3) / 1e12, "colour_kernel_TB_per_s": colour_bytes / (colour_ms * 1e-3) / 1e12,
                "idct_fraction_of_hbm_peak": idct_bytes / (idct_ms * 1e-3) / HBM_PEAK_MEASURED,
                "colour_fraction_of_hbm_peak": colour_bytes / (colour_ms * 1e-3) / HBM_PEAK_MEASURED,
                "uploaded_bytes_per_image_A": 480 * 640 * 3, "uploaded_bytes_per_image_B": need / m + ctypes.sizeof(JpegDesc) + 8})
    # ---- the split of route C on the same views --------------------------------------------------------------------------------------
    from poem_v2_amd.jpeg import HUFF_BYTES, JpegScan
    scans, t8 = (JpegScan * m)(), (ctypes.c_int64 * 8)()
    hip.check(L.poem_jpeg_entropy_prepare(ptrs, lens, m, a.subseq, descs, scans, None, 0, None, 0, t8))
    ntab, packed_need, subs = int(t8[5]), int(t8[4]), int(t8[6])
    side = torch.empty(ntab * HUFF_BYTES + packed_need, dtype=torch.uint8, pin_memory=True)
    ts = []
    for _ in range(a.reps + 1):
        t0 = time.perf_counter()
        hip.check(L.poem_jpeg_entropy_prepare(ptrs, lens, m, a.subseq, descs, scans, None, 0, None, 0, t8))
        hip.check(L.poem_jpeg_entropy_prepare(ptrs, lens, m, a.subseq, descs, scans, side.data_ptr(), ntab,
                                              side.data_ptr() + ntab * HUFF_BYTES, packed_need, t8))
        ts.append(time.perf_counter() - t0)
    res["C_prepare_ms_per_image"] = statistics.median(ts[1:]) * 1e3 / m
    sdev = torch.empty_like(side, device=dev)
    ddev2 = torch.frombuffer(bytearray(bytes(descs)), dtype=torch.uint8).to(dev)
    scdev = torch.frombuffer(bytearray(bytes(scans)), dtype=torch.uint8).to(dev)
    status = torch.empty(m, dtype=torch.int32, device=dev)
    work = torch.empty(L.poem_jpeg_entropy_workspace_bytes(m, subs), dtype=torch.uint8, device=dev)

    def entropy(total_blocks):
        hip.check(L.poem_jpeg_entropy_device(ddev2.data_ptr(), scdev.data_ptr(), sdev.data_ptr(), ntab, sdev.data_ptr() + ntab * HUFF_BYTES,
                                             packed_need, m, a.subseq, a.wg_threads, subs, total_blocks, cdev.data_ptr(), need,
                                             status.data_ptr(), work.data_ptr(), work.numel(), hip.stream()))

    up_packed_ms = events(lambda: sdev.copy_(side, non_blocking=True))
    zero_ms = events(lambda: cdev.zero_())
    decode_ms = events(lambda: entropy(0))                     # memset + decode kernel: the range-guard kernel has no block to visit
    whole_ms = events(lambda: entropy(blocks))
    ts = []
    for _ in range(a.reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        got = status.cpu()
        ts.append(time.perf_counter() - t0)
    assert int(got.abs().sum()) == 0, "the device refused a benchmark view"
    check = torch.empty(need, dtype=torch.uint8, device=dev)
    check.copy_(pinned)                                          # the host threads' coefficients (decoded above)
    assert torch.equal(check, cdev), "device coefficients differ from the host decoder's"
    recon(quads)
    rounds = work[:4 * m].cpu().numpy().view(np.int32)
    hist = {}
    for r in rounds.tolist():
        hist[r] = hist.get(r, 0) + 1
    res.update({"C_upload_packed_ms_per_image": up_packed_ms / m, "C_memset_ms_per_image": zero_ms / m,
                "C_decode_kernel_ms_per_image": max(decode_ms - zero_ms, 0.0) / m,
                "C_range_guard_kernel_ms_per_image": max(whole_ms - decode_ms, 0.0) / m, "C_entropy_launch_ms_per_image": whole_ms / m,
                "C_status_readback_ms_per_call": statistics.median(ts[1:]) * 1e3, "C_reconstruct_ms_per_image": both_ms / m,
                "C_rounds_histogram": {str(k): hist[k] for k in sorted(hist)}, "C_subsequences_per_image": subs / m,
                "uploaded_bytes_per_image_C": (packed_need + ntab * HUFF_BYTES) / m + ctypes.sizeof(JpegDesc) + ctypes.sizeof(JpegScan) + 8})
    print(json.dumps(res))


if __name__ == "__main__":
    main()
