"""The image kernels at every border, stride and alignment path, bit for bit against the oracle (tests/test_image_cases_cpu.py pins that oracle to NumPy models at
the same sizes).  csrc/image.hip chooses its load and store paths by width, height, row stride, batch stride and pointer alignment:

  pyr_down_u8_kernel    loads: the whole-wave dword path (h >= 8, every lane's first two dwords inside the row), the per-row dword path with byte selectors for the
                        left border and the right edge, the per-byte path (w < 16, or the second dword crosses the edge), rows reflected more than once (h < 8);
                        stores: a dword, or bytes when the row stride, the batch stride or the base is no multiple of 4; workgroups dealt in XCD-contiguous order or not
  convert_sobel_kernel  stores: float4, or scalars for a partial group of 4, a row or batch stride that is no multiple of 4 floats, or an output that is not
                        16-byte aligned
  svs_preprocess_gpu_sem (csrc/dense_full.hip)  three one-lane-per-pixel kernels, any w, h >= 1

Every call goes through the public C ABI on torch device buffers.  Destinations are filled with a canary first and every element outside the images must keep it;
sources with padding are run twice, padding 255 and padding 0, and must give the same bytes (padding may be read, never used).
Each test loops over its sizes inside one test item and reuses one set of buffers sized for its largest case."""
import ctypes as C
import time

import numpy as np
import pytest

import image_cases as IC

pytestmark = pytest.mark.gpu

_REF = {}


def _ref(kind, w, h):
    """the oracle's answer for IC.images(w, h), computed once per size and shared read-only"""
    import oracle as O
    key = (kind, w, h)
    if key not in _REF:
        imgs = IC.images(w, h)
        if kind == "pyr":
            r = np.stack([O.pyr_down_u8(i) for i in imgs])
        elif kind == "sobel":
            r = np.stack([np.stack(O.convert_sobel(i)) for i in imgs])          # [image, (img, dx, dy), h, w]
        else:
            r = [O.preprocess_gpu_sem(i, 3) for i in imgs]                         # [image][(img, dx, dy)][level]
        if isinstance(r, np.ndarray):
            r.setflags(write=False)
        _REF[key] = r
    return _REF[key]


def _pyr_call(ctx, src, sp, dst, dp):
    ctx.call("svs_pyr_down_u8", src.ptr(sp), sp.w, sp.h, sp.stride, sp.bstride, dst.ptr(dp), dp.stride, dp.bstride, sp.n)
    ctx.sync()
    return dst.download()


def _pyr_buffers(geo):
    return IC.DeviceBuffer(max(s.size for s, d in geo), 0), IC.DeviceBuffer(max(d.size for s, d in geo), IC.U8_CANARY)


@pytest.mark.parametrize("layout", IC.PYR_LAYOUTS)
def test_pyr_down_every_size_and_layout(gpu_ctx, layout):
    """One svs_pyr_down_u8 call per size of IC.PYR_SIZES with the five images as the batch: every output equals the oracle's, every byte of the destination outside
    the dw x dh images keeps the canary (row padding, the rows between images, the bytes before an offset base and behind the last image), and -- layouts with
    padding -- the destination is the same byte for byte whether the source's padding holds 255 or 0."""
    import torch
    ctx, stream = gpu_ctx
    t0, n, cases = time.perf_counter(), 5, 0
    geo = {s: IC.pyr_layout(layout, s[0], s[1], n) for s in IC.PYR_SIZES}
    with torch.cuda.stream(stream):
        src, dst = _pyr_buffers(geo.values())
        for (w, h), (sp, dp) in geo.items():
            imgs, ref, flats = IC.images(w, h), _ref("pyr", w, h), []
            for pad in (255,) if layout == "tight" else (255, 0):
                src.upload(sp.pack(imgs, pad, src.t.numel()))
                dst.fill()
                flat = _pyr_call(ctx, src, sp, dst, dp)
                got = dp.unpack(flat)
                for b in range(n):
                    assert np.array_equal(got[b], ref[b]), (layout, w, h, b, pad, np.argwhere(got[b] != ref[b])[:4].tolist())
                    cases += 1
                assert (dp.outside(flat) == IC.U8_CANARY).all(), (layout, w, h, pad, "canary overwritten")
                flats.append(flat)
            assert len(flats) == 1 or np.array_equal(flats[0], flats[1]), (layout, w, h, "the result depends on the source's padding")
    print(f"pyr_down {layout}: {cases} (size, layout, image) cases in {time.perf_counter() - t0:.2f} s")


def test_pyr_down_swizzle_and_many_workgroups(gpu_ctx):
    """3 and 9 workgroups per image, batches of 3 and 4 (9, 12, 27, 36 workgroups: none a multiple of the 8 XCDs), with the XCD-contiguous workgroup order off and on:
    both equal the oracle, and so each other."""
    import torch
    ctx, stream = gpu_ctx
    t0, cases, pick = time.perf_counter(), 0, [IC.NOISE, IC.RAMP, IC.CHECKER, IC.WHITE]
    geo = {(s, layout, n): IC.pyr_layout(layout, s[0], s[1], n) for s in IC.PYR_SWIZZLE_SIZES for layout in ("pitched", "tight") for n in (3, 4)}
    try:
        with torch.cuda.stream(stream):
            src, dst = _pyr_buffers(geo.values())
            for ((w, h), layout, n), (sp, dp) in geo.items():
                imgs, ref, flats = IC.images(w, h)[pick[:n]], _ref("pyr", w, h)[pick[:n]], []
                src.upload(sp.pack(imgs, 255, src.t.numel()))
                for swz in (0, 1):
                    ctx.set_option("xcd_swizzle", swz)
                    dst.fill()
                    flat = _pyr_call(ctx, src, sp, dst, dp)
                    assert np.array_equal(dp.unpack(flat), ref), (w, h, layout, n, swz)
                    assert (dp.outside(flat) == IC.U8_CANARY).all(), (w, h, layout, n, swz, "canary overwritten")
                    flats.append(flat)
                    cases += n
                assert np.array_equal(flats[0], flats[1])
    finally:
        ctx.set_option("xcd_swizzle", 1)
    print(f"pyr_down swizzle: {cases} (size, layout, image) cases in {time.perf_counter() - t0:.2f} s")


def test_pyr_down_chain_to_one_pixel_row(gpu_ctx):
    """The pitch hand-over between levels as include/scavislam_hip.hpp does it (64-byte pitch, batch stride 0, one image): 41 x 11 noise, the call applied to its own
    output while the source still has 3 rows and columns (41 x 11 -> 21 x 6 -> 11 x 3 -> 6 x 2).  Every level equals the oracle's step on the oracle's previous level."""
    import torch
    import oracle as O
    ctx, stream = gpu_ctx
    t0, w, h = time.perf_counter(), 41, 11
    ref, levels = IC.images(w, h)[IC.NOISE], 0
    with torch.cuda.stream(stream):
        plane = IC.Plane(w, h, 1, 0, IC.round_up(w, 64), 0)
        cur = IC.DeviceBuffer(plane.size, IC.U8_CANARY)
        cur.upload(plane.pack(ref[None], IC.U8_CANARY))
        while plane.w >= 3 and plane.h >= 3:
            nxt_plane = IC.Plane(IC.half(plane.w), IC.half(plane.h), 1, 0, IC.round_up(IC.half(plane.w), 64), 0)
            nxt = IC.DeviceBuffer(nxt_plane.size, IC.U8_CANARY)
            nxt.fill()
            flat = _pyr_call(ctx, cur, plane, nxt, nxt_plane)
            ref = O.pyr_down_u8(ref)
            assert np.array_equal(nxt_plane.unpack(flat)[0], ref), (plane.w, plane.h)
            assert (nxt_plane.outside(flat) == IC.U8_CANARY).all(), (plane.w, plane.h, "canary overwritten")
            cur, plane, levels = nxt, nxt_plane, levels + 1
    assert levels == 3 and ref.shape == (2, 6)
    print(f"pyr_down chain: {levels} (size, layout, image) cases in {time.perf_counter() - t0:.2f} s")


@pytest.mark.parametrize("layout", IC.SOBEL_LAYOUTS)
def test_convert_sobel_every_size_and_layout(gpu_ctx, layout):
    """One svs_convert_sobel_f32 call per size of IC.SOBEL_SIZES, batch of 3 (noise, all 255, ramp): img, dx, dy equal the oracle's; every word of the three float
    buffers outside the images keeps the canary's bit pattern; the outputs do not depend on the source's padding.  "tight" and "skewed" reach the scalar store path
    through the row / batch stride, "skew_img" / "skew_dx" / "skew_dy" through the alignment of exactly one of the three output pointers."""
    import torch
    ctx, stream = gpu_ctx
    t0, cases, pick = time.perf_counter(), 0, [IC.NOISE, IC.WHITE, IC.RAMP]
    geo = {s: IC.sobel_layout(layout, s[0], s[1], 3) for s in IC.SOBEL_SIZES}
    with torch.cuda.stream(stream):
        src = IC.DeviceBuffer(max(sp.size for sp, _ in geo.values()), 0)
        outs = [IC.DeviceBuffer(max(fp[k].size for _, fp in geo.values()), IC.F32_CANARY, words=True) for k in range(3)]
        for (w, h), (sp, fp) in geo.items():
            imgs, ref, runs = IC.images(w, h)[pick], _ref("sobel", w, h)[pick], []
            assert len({(p.stride, p.bstride) for p in fp}) == 1
            for pad in (255,) if layout == "tight" else (255, 0):
                src.upload(sp.pack(imgs, pad, src.t.numel()))
                for o in outs:
                    o.fill()
                ctx.call("svs_convert_sobel_f32", src.ptr(sp), w, h, sp.stride, sp.bstride, outs[0].ptr(fp[0]), outs[1].ptr(fp[1]), outs[2].ptr(fp[2]),
                         fp[0].stride, fp[0].bstride, 3)
                ctx.sync()
                flats = [o.download() for o in outs]
                for k, name in enumerate(("img", "dx", "dy")):
                    got = fp[k].unpack(flats[k]).view(np.float32)
                    for b in range(3):
                        assert np.array_equal(got[b], ref[b, k]), (layout, w, h, name, b, pad, np.argwhere(got[b] != ref[b, k])[:4].tolist())
                    assert (fp[k].outside(flats[k]) == IC.F32_CANARY).all(), (layout, w, h, name, pad, "canary overwritten")
                cases += 3
                runs.append(flats)
            assert len(runs) == 1 or all(np.array_equal(a, b) for a, b in zip(*runs)), (layout, w, h, "the result depends on the source's padding")
    print(f"convert_sobel {layout}: {cases} (size, layout, image) cases in {time.perf_counter() - t0:.2f} s")


def test_preprocess_gpu_sem_tiny_and_padded(gpu_ctx):
    """svs_preprocess_gpu_sem at IC.F32_SIZES, 1 to 3 levels, batch of 2, odd source base and strides, fstride[l] = lw + 3 and f_bstride[l] = fstride[l] * lh + 7:
    every level's img, dx, dy equal the oracle's, and the canary words of all nine output buffers stay untouched (the buffers of levels that are not asked for whole)."""
    import torch
    ctx, stream = gpu_ctx
    t0, cases, pick = time.perf_counter(), 0, [IC.NOISE, IC.RAMP]
    geo = {(s, levels): IC.f32_layout(s[0], s[1], levels, 2) for s in IC.F32_SIZES for levels in (1, 2, 3)}
    P = C.c_void_p * 3
    with torch.cuda.stream(stream):
        src = IC.DeviceBuffer(max(sp.size for sp, _ in geo.values()), 0)
        size = [max(fp[l].size for _, fp in geo.values() if len(fp) > l) for l in range(3)]
        outs = [[IC.DeviceBuffer(size[l], IC.F32_CANARY, words=True) for l in range(3)] for _ in range(3)]       # [img, dx, dy][level]
        for ((w, h), levels), (sp, fp) in geo.items():
            imgs, ref = IC.images(w, h)[pick], [_ref("f32", w, h)[b] for b in pick]
            src.upload(sp.pack(imgs, 255, src.t.numel()))
            for o in outs:
                for buf in o:
                    buf.fill()
            ptrs = [P(*[outs[k][l].ptr(fp[l]) if l < levels else None for l in range(3)]) for k in range(3)]
            ctx.call("svs_preprocess_gpu_sem", src.ptr(sp), w, h, sp.stride, sp.bstride, ptrs[0], ptrs[1], ptrs[2],
                     (C.c_int32 * 3)(*[fp[l].stride if l < levels else 0 for l in range(3)]), (C.c_size_t * 3)(*[fp[l].bstride if l < levels else 0 for l in range(3)]), levels, 2)
            ctx.sync()
            for k, name in enumerate(("img", "dx", "dy")):
                for l in range(3):
                    flat = outs[k][l].download()
                    if l >= levels:
                        assert (flat == IC.F32_CANARY).all(), (w, h, levels, name, l, "a level that was not asked for was written")
                        continue
                    got = fp[l].unpack(flat).view(np.float32)
                    for b in range(2):
                        assert np.array_equal(got[b], ref[b][k][l]), (w, h, levels, name, l, b)
                    assert (fp[l].outside(flat) == IC.F32_CANARY).all(), (w, h, levels, name, l, "canary overwritten")
            cases += 2 * levels
    print(f"preprocess_gpu_sem: {cases} (size, level, image) cases in {time.perf_counter() - t0:.2f} s")


def test_image_calls_reject_what_they_cannot_do(gpu_ctx):
    """Sizes below a kernel's footprint, a level whose row stride is shorter than its width and an empty batch are refused before anything is launched: the call
    raises, and a canary-filled destination is untouched byte for byte."""
    import torch
    from scavislam_amd import capi
    ctx, stream = gpu_ctx
    P = C.c_void_p * 3
    with torch.cuda.stream(stream):
        src = IC.DeviceBuffer(4096, 0)
        dst8 = IC.DeviceBuffer(4096, IC.U8_CANARY)
        f = [IC.DeviceBuffer(4096, IC.F32_CANARY, words=True) for _ in range(9)]
        src.upload(np.arange(4096, dtype=np.uint8))
        p8, pf = dst8.t.data_ptr(), [b.t.data_ptr() for b in f]

        def pyr(w, h, batch):
            ctx.call("svs_pyr_down_u8", src.t.data_ptr(), w, h, 16, 256, p8, 16, 256, batch)

        def sobel(w, h, batch):
            ctx.call("svs_convert_sobel_f32", src.t.data_ptr(), w, h, 16, 256, pf[0], pf[1], pf[2], 16, 256, batch)

        def pre(fstride, batch):          # 9 x 5, three levels: 9, 5, 3 columns
            ctx.call("svs_preprocess_gpu_sem", src.t.data_ptr(), 9, 5, 16, 256, P(*pf[0:3]), P(*pf[3:6]), P(*pf[6:9]), (C.c_int32 * 3)(*fstride),
                     (C.c_size_t * 3)(256, 256, 256), 3, batch)

        for what, fn in (("pyr w = 2", lambda: pyr(2, 8, 2)), ("pyr h = 2", lambda: pyr(8, 2, 2)), ("pyr batch = 0", lambda: pyr(8, 8, 0)),
                         ("sobel w = 1", lambda: sobel(1, 8, 2)), ("sobel batch = 0", lambda: sobel(8, 8, 0)),
                         ("preprocess fstride[1] < lw", lambda: pre((16, 4, 16), 2)), ("preprocess fstride[2] < lw", lambda: pre((16, 16, 2), 2)),
                         ("preprocess batch = 0", lambda: pre((16, 16, 16), 0))):
            dst8.fill()
            for b in f:
                b.fill()
            with pytest.raises(capi.SvsError):
                fn()
            ctx.sync()
            assert (dst8.download() == IC.U8_CANARY).all(), what
            for b in f:
                assert (b.download() == IC.F32_CANARY).all(), what
