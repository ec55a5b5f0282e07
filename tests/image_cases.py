"""Sizes, images and buffer layouts shared by tests/test_image_cases_cpu.py and tests/test_gpu_image_edges.py: the cases at which the image kernels
(csrc/image.hip: the u8 pyramid step, the f32 convert + Sobel; csrc/dense_full.hip: the CUDA-branch preprocessing) choose another load or store path.
Plain data and host-side helpers; the device buffers are torch tensors and nothing here launches a kernel.

A `Plane` places a batch of equally sized 2-D images in one flat buffer: image b, row y, column x lies at element  off + b * bstride + y * stride + x.
Everything else in the buffer is padding -- of a source it is filled with a value the result must not depend on, of a destination with a canary that must survive."""
import numpy as np

# ---- sizes ---------------------------------------------------------------------------------------------------------------------------------------------------
# pyramid step (w, h >= 3): every width residue mod 8 on both sides of the per-byte / dword threshold (w = 16) and of the row-path threshold (h = 8); one and two
# dwords per footprint row crossing the right edge; a few widths around one and two waves of lanes; two sizes whose workgroup count (3 and 9 per image) times
# a batch of 3 or 4 is no multiple of the 8 XCDs
PYR_SIZES = ([(w, h) for w in range(3, 42) for h in range(3, 12)] + [(w, h) for w in (63, 64, 65, 127, 129) for h in (8, 9, 15, 17)] + [(200, 100), (1030, 66)])
PYR_SWIZZLE_SIZES = [(200, 100), (1030, 66)]
# convert + Sobel (w, h >= 2): a lane covers 4 pixels of a row and a block 256; full and partial groups of 4 on both sides of one block
SOBEL_SIZES = [(w, h) for w in list(range(2, 22)) + list(range(63, 68)) + list(range(255, 262)) for h in (2, 3, 4, 7)]
# CUDA-branch preprocessing (w, h >= 1): one lane per pixel; levels that shrink to a single row, column or pixel
F32_SIZES = [(w, h) for w in (1, 2, 3, 4, 5, 7, 9, 13, 65, 129) for h in (1, 2, 3, 4, 5, 9)]

U8_CANARY = 0xA5
F32_CANARY = 0x7FC0A5A5          # a NaN's bit pattern: no image value compares equal to it, and the buffers are compared as uint32

PYR_LAYOUTS = ("tight", "pitched", "skewed")
SOBEL_LAYOUTS = ("tight", "pitched", "skewed", "skew_img", "skew_dx", "skew_dy")


def round_up(n, m):
    return (n + m - 1) // m * m


def half(n):
    return (n + 1) // 2


def images(w, h):
    """[5, h, w] u8: seeded noise, all 255, all 0, a 0 / 255 checkerboard, and the ramp (7 x + 13 y) & 255 -- every column and every row inside a
    5 x 5 (or 7 x 11) footprint of the ramp is different from the others, so a wrong byte selector or row index cannot cancel."""
    yy, xx = np.mgrid[0:h, 0:w]
    noise = np.random.default_rng(4099 * w + h).integers(0, 256, (h, w))
    return np.stack([noise, np.full((h, w), 255), np.zeros((h, w), np.int64), ((xx + yy) & 1) * 255, (7 * xx + 13 * yy) & 255]).astype(np.uint8)


NOISE, WHITE, BLACK, CHECKER, RAMP = range(5)


# ---- layouts -------------------------------------------------------------------------------------------------------------------------------------------------
class Plane:
    """n images of w x h elements in a flat buffer of `size` elements (see the module docstring); `off` is counted from an allocation's own (aligned) base."""

    def __init__(self, w, h, n, off, stride, bstride):
        assert stride >= w and (n == 1 or bstride >= stride * (h - 1) + w)
        self.w, self.h, self.n, self.off, self.stride, self.bstride = w, h, n, off, stride, bstride
        self.size = off + (n - 1) * bstride + (h - 1) * stride + w + 16      # (16 elements behind the last image: its canary)

    def _index(self):
        b, y, x = np.ogrid[0:self.n, 0:self.h, 0:self.w]
        return self.off + b * self.bstride + y * self.stride + x

    def pack(self, imgs, fill, size=None):
        """flat host buffer of `size` elements (default: the plane's own) holding `imgs` [n, h, w], `fill` everywhere else"""
        imgs = np.asarray(imgs)
        assert imgs.shape == (self.n, self.h, self.w)
        flat = np.full(size or self.size, fill, imgs.dtype)
        flat[self._index()] = imgs
        return flat

    def unpack(self, flat):
        return flat[self._index()]

    def outside(self, flat):
        """every element of the flat buffer that belongs to no image"""
        keep = np.ones(len(flat), bool)
        keep[self._index().ravel()] = False
        return flat[keep]


def pyr_layout(name, w, h, n):
    """(source plane, destination plane) of one svs_pyr_down_u8 call, in bytes"""
    dw, dh = half(w), half(h)
    if name == "tight":                      # stride = width: rows and images at every alignment, the allocation's own base
        return Plane(w, h, n, 0, w, w * h), Plane(dw, dh, n, 0, dw, dw * dh)
    if name == "pitched":                    # what the library's own pyramids use: 64-byte pitch, three rows between images
        ss, ds = round_up(w, 64), round_up(dw, 64)
        return Plane(w, h, n, 0, ss, ss * (h + 3)), Plane(dw, dh, n, 0, ds, ds * (dh + 3))
    if name == "skewed":                     # odd base, odd strides; a destination whose rows are dword-pitched but whose base and batch stride are not
        ss, ds = w + 3, round_up(dw, 4)
        return Plane(w, h, n, 1, ss, ss * h + 5), Plane(dw, dh, n, 1, ds, ds * dh + 2)
    raise ValueError(name)


def sobel_layout(name, w, h, n):
    """(source plane in bytes, [img, dx, dy] planes in floats) of one svs_convert_sobel_f32 call; the three outputs share stride and batch stride"""
    if name == "tight":
        src, off, fs, fb = Plane(w, h, n, 0, w, w * h), (0, 0, 0), w, w * h
    elif name == "pitched":
        ss, fs = round_up(w, 64), round_up(w, 64)
        src, off, fb = Plane(w, h, n, 0, ss, ss * (h + 3)), (0, 0, 0), fs * (h + 3)
    elif name == "skewed":                   # rows 16-byte pitched, the batch stride alone is odd
        fs = round_up(w, 4)
        src, off, fb = Plane(w, h, n, 1, w + 3, (w + 3) * h + 5), (0, 0, 0), fs * h + 1
    elif name in ("skew_img", "skew_dx", "skew_dy"):      # strides 16-byte multiples; exactly ONE output starts 4 bytes past a 16-byte boundary
        ss, fs = round_up(w, 64), round_up(w, 4)
        src, fb = Plane(w, h, n, 0, ss, ss * (h + 3)), fs * h
        off = tuple(1 if name == "skew_" + k else 0 for k in ("img", "dx", "dy"))
    else:
        raise ValueError(name)
    return src, [Plane(w, h, n, o, fs, fb) for o in off]


def f32_layout(w, h, levels, n):
    """(source plane, [per level: the plane the level's img / dx / dy buffers share]) of one svs_preprocess_gpu_sem call: odd row strides, odd batch strides"""
    src = Plane(w, h, n, 1, w + 3, (w + 3) * h + 5)
    planes, lw, lh = [], w, h
    for _ in range(levels):
        planes.append(Plane(lw, lh, n, 0, lw + 3, (lw + 3) * lh + 7))
        lw, lh = half(lw), half(lh)
    return src, planes


# ---- device buffers ------------------------------------------------------------------------------------------------------------------------------------------
class DeviceBuffer:
    """One torch allocation of `size` elements (u8, or 32-bit words for the float planes), reused by every case of a test and re-filled on the device."""

    def __init__(self, size, canary, words=False):
        import torch
        self.t = torch.empty(int(size), dtype=torch.int32 if words else torch.uint8, device="cuda")
        self.canary, self.words = canary, words
        assert self.t.data_ptr() % 256 == 0      # the allocation's own base: what `Plane.off` is counted from

    def ptr(self, plane):
        return self.t.data_ptr() + plane.off * (4 if self.words else 1)

    def fill(self):
        self.t.fill_(self.canary)

    def upload(self, flat):
        import torch
        assert len(flat) <= self.t.numel()
        self.t[:len(flat)].copy_(torch.from_numpy(flat.view(np.int32) if self.words else flat))

    def download(self):
        a = self.t.cpu().numpy()
        return a.view(np.uint32) if self.words else a
