"""The yardstick of tests/test_gpu_image_edges.py, pinned on the CPU: at every size of tests/image_cases.py the C oracle of the image kernels equals an
independent NumPy model written from the definitions (tests/np_model.py).  A later change to the oracle cannot silently move what the GPU tests compare with."""
import numpy as np

import image_cases as IC
import np_model


def test_case_lists_hold_what_the_kernels_branch_on():
    pyr, sob, f32 = set(IC.PYR_SIZES), set(IC.SOBEL_SIZES), set(IC.F32_SIZES)
    assert len(pyr) == len(IC.PYR_SIZES) == 39 * 9 + 5 * 4 + 2 and len(sob) == len(IC.SOBEL_SIZES) == 32 * 4 and len(f32) == len(IC.F32_SIZES) == 60
    assert {w % 8 for w, h in pyr if w < 16} == {w % 8 for w, h in pyr if 16 <= w <= 41} == set(range(8))
    assert {h for w, h in pyr if w <= 41} == set(range(3, 12))
    # workgroups of 256 lanes, one lane per 4 x 2 outputs: 3 and 9 per image, so 9 and 36 for a batch of 3 and 4
    wgs = {(w, h): IC.round_up(IC.round_up(IC.half(w), 4) // 4 * (IC.round_up(IC.half(h), 2) // 2), 256) // 256 for w, h in IC.PYR_SWIZZLE_SIZES}
    assert wgs == {(200, 100): 3, (1030, 66): 9} and all(s in pyr for s in wgs)
    assert {w % 4 for w, h in sob} == set(range(4)) and {255, 256, 257} <= {w for w, h in sob}


def test_images_and_planes():
    im = IC.images(13, 5)
    assert im.shape == (5, 5, 13) and im.dtype == np.uint8
    assert (im[IC.WHITE] == 255).all() and (im[IC.BLACK] == 0).all() and set(np.unique(im[IC.CHECKER])) == {0, 255}
    ramp = IC.images(41, 11)[IC.RAMP]
    assert all(len(set(ramp[0, x:x + 11])) == 11 for x in range(31)) and all(len(set(ramp[y:y + 7, 0])) == 7 for y in range(5))
    for name in IC.PYR_LAYOUTS:
        for plane in IC.pyr_layout(name, 13, 5, 5):
            imgs = np.random.default_rng(1).integers(0, 256, (5, plane.h, plane.w)).astype(np.uint8)
            flat = plane.pack(imgs, 7)
            assert np.array_equal(plane.unpack(flat), imgs) and (plane.outside(flat) == 7).all()
            assert len(plane.outside(flat)) == plane.size - imgs.size and plane.outside(flat).size >= 16
    src, dst = IC.pyr_layout("skewed", 13, 5, 5)
    assert (src.off, src.stride, src.bstride) == (1, 16, 85) and (dst.off, dst.stride, dst.bstride) == (1, 8, 26)
    for k, name in enumerate(("skew_img", "skew_dx", "skew_dy")):
        _, outs = IC.sobel_layout(name, 13, 5, 3)
        assert [p.off for p in outs] == [int(j == k) for j in range(3)] and outs[0].stride % 4 == 0 and outs[0].bstride % 4 == 0
    _, outs = IC.sobel_layout("skewed", 13, 5, 3)
    assert outs[0].stride % 4 == 0 and outs[0].bstride % 4 == 1


def test_pyr_down_oracle_equals_model_at_every_size():
    import oracle as O
    n = 0
    for w, h in IC.PYR_SIZES:
        for k, img in enumerate(IC.images(w, h)):
            got = O.pyr_down_u8(img)
            assert got.shape == (IC.half(h), IC.half(w)) and np.array_equal(got, np_model.pyr_down(img)), (w, h, k)
            n += 1
    assert n == 5 * len(IC.PYR_SIZES)


def test_convert_sobel_oracle_equals_model_at_every_size():
    import oracle as O
    for w, h in IC.SOBEL_SIZES:
        for k, img in enumerate(IC.images(w, h)):
            f, dx, dy = O.convert_sobel(img)
            f_ref = img.astype(np.float32) * np.float32(1. / 255.)
            dx_ref, dy_ref = np_model.sobel(f_ref)
            assert f.dtype == dx.dtype == dy.dtype == np.float32
            assert np.array_equal(f, f_ref) and np.array_equal(dx, dx_ref) and np.array_equal(dy, dy_ref), (w, h, k)


def test_preprocess_gpu_sem_oracle_equals_model_at_every_size():
    import oracle as O
    for w, h in IC.F32_SIZES:
        img = IC.images(w, h)[IC.NOISE]
        f, dx, dy = O.preprocess_gpu_sem(img, 3)
        ref = img.astype(np.float32) * np.float32(1. / 255.)
        for l in range(3):
            if l:
                ref = np_model.pyr_down_f32(ref)
            dx_ref, dy_ref = np_model.deriv_replicate(ref)
            assert f[l].shape == ref.shape and f[l].dtype == np.float32
            assert np.array_equal(f[l], ref) and np.array_equal(dx[l], dx_ref) and np.array_equal(dy[l], dy_ref), (w, h, l)
