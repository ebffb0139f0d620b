"""Helper (no tests): a numpy restatement of the clip augmentation ops alpro_augment_stage runs on the device, written from the
op definitions, not from the reference's OpenCV calls, plus the shapes, images and levels the tests share.

A frame is (3, H, W) uint8, channels in stored order.  Bilinear ops and Color are evaluated in fp64; the pointwise ops in the
precision their definition states (Brightness and the Sharpness blend in fp32 with one rounding per operation, the Contrast
table in fp64, everything else in integers)."""
import numpy as np

FILL = 128
OPS = {"Identity": 0, "HorizontalFlip": 1, "Brightness": 2, "Contrast": 3, "Sharpness": 4, "Color": 5, "Solarize": 6, "Posterize": 7,
       "TranslateX": 8, "TranslateY": 9, "ShearX": 10, "ShearY": 11, "Rotate": 12}
NAMES = {v: k for k, v in OPS.items()}
EXACT_OPS = ["Identity", "HorizontalFlip", "Brightness", "Contrast", "Sharpness", "Solarize", "Posterize", "TranslateX", "TranslateY"]
CLOSE_OPS = ["ShearX", "ShearY", "Rotate", "Color"]          # <= 1 grey level, <= 5 % of the elements
SHAPES = [(37, 53), (64, 64), (16, 200)]
LEVELS = [3, 5, 8]
B, T = 3, 2


def enhance_factor(M):
    return M / 10 * 1.8 + 0.1


def images(H, W):
    """{'noise': seeded uniform noise, 'ramp': a smooth two-way ramp, different per channel}, each (3, H, W) uint8."""
    rng = np.random.RandomState(1000 * H + W)
    y, x = np.mgrid[0:H, 0:W]
    ramp = np.stack([(x * 255) // max(W - 1, 1), (y * 255) // max(H - 1, 1), ((x + y) * 255) // max(H + W - 2, 1)]).astype(np.uint8)
    return {"noise": rng.randint(0, 256, (3, H, W)).astype(np.uint8), "ramp": ramp}


def _warp(img, sx, sy):
    """dst(x, y) = src(sx, sy): the four taps around the fp64 position, FILL for a tap outside the image, rounded to nearest."""
    C, H, W = img.shape
    x0, y0 = np.floor(sx).astype(np.int64), np.floor(sy).astype(np.int64)
    wx, wy = sx - x0, sy - y0

    def tap(xi, yi):
        ok = (xi >= 0) & (xi < W) & (yi >= 0) & (yi < H)
        v = img[:, np.clip(yi, 0, H - 1), np.clip(xi, 0, W - 1)].astype(np.float64)
        return np.where(ok[None], v, float(FILL))
    v00, v01, v10, v11 = tap(x0, y0), tap(x0 + 1, y0), tap(x0, y0 + 1), tap(x0 + 1, y0 + 1)
    top = v00 + wx * (v01 - v00)
    bot = v10 + wx * (v11 - v10)
    return np.clip(np.floor(top + wy * (bot - top) + 0.5), 0, 255).astype(np.uint8)


def degenerate(img):
    """3x3 correlation with [[1,1,1],[1,5,1],[1,1,1]] / 13 over a reflect-101 border, rounded to nearest (S / 13 is never a tie)."""
    C, H, W = img.shape
    p = np.pad(img.astype(np.int64), ((0, 0), (1, 1), (1, 1)), mode="reflect")
    S = sum(p[:, dy:dy + H, dx:dx + W] for dy in range(3) for dx in range(3)) + 4 * p[:, 1:1 + H, 1:1 + W]
    return ((2 * S + 13) // 26).astype(np.uint8)


def apply_op(img, name, M):
    """One op on one (3, H, W) uint8 frame at level M -> (3, H, W) uint8."""
    C, H, W = img.shape
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    f = enhance_factor(M)
    if name == "Identity":
        return img.copy()
    if name == "HorizontalFlip":
        return img[:, :, ::-1].copy()
    if name == "Brightness":
        table = np.clip(np.arange(256, dtype=np.float32) * np.float32(f), 0, 255).astype(np.uint8)
        return table[img]
    if name == "Contrast":
        n = H * W
        m = [np.float64(int(img[c].astype(np.int64).sum())) / np.float64(n) for c in range(3)]
        mean = (m[0] * 0.114 + m[1] * 0.587) + m[2] * 0.299
        table = np.clip((np.arange(256, dtype=np.float64) - mean) * f + mean, 0, 255).astype(np.uint8)
        return table[img]
    if name == "Sharpness":
        deg = degenerate(img)
        if f == 1.0:
            return img.copy()
        if f == 0.0:
            return deg
        out = img.copy()
        s32, d32 = img.astype(np.float32), deg.astype(np.float32)
        blend = d32 + np.float32(f) * (s32 - d32)                      # fp32, one rounding per operation
        out[:, 1:-1, 1:-1] = np.clip(blend, 0, 255).astype(np.uint8)[:, 1:-1, 1:-1]   # clamp where f > 1 leaves 0..255
        return out
    if name == "Color":
        w = np.array([0.114, 0.587, 0.299])
        m3 = (np.eye(3) - w[:, None]) * f + w[:, None]                  # m3[i][j] = A[i][j] * f + w[i], A = I - w 1^T
        out = np.einsum("ihw,ij->jhw", img.astype(np.float64), m3)
        return np.clip(out, 0, 255).astype(np.uint8)
    if name == "Solarize":
        t = int(M / 10 * 256)
        return np.where(img < t, img, 255 - img).astype(np.uint8)
    if name == "Posterize":
        b = int(M / 10 * 4)
        return img & np.uint8((255 << (8 - b)) & 255)
    if name == "TranslateX":
        return _warp(img, x + M / 10 * 10.0, y)
    if name == "TranslateY":
        return _warp(img, x, y + M / 10 * 10.0)
    if name == "ShearX":
        return _warp(img, x - (M / 10 * 0.3) * y, y)
    if name == "ShearY":
        return _warp(img, x, y - (M / 10 * 0.3) * x)
    if name == "Rotate":
        d = np.deg2rad(M / 10 * 30)
        a, b, cx, cy = np.cos(d), np.sin(d), W / 2, H / 2
        r = np.array([[a, b, (1 - a) * cx - b * cy], [-b, a, b * cx + (1 - a) * cy], [0, 0, 1]])
        ri = np.linalg.inv(r)                                            # dst(p) = src(R^-1 p)
        return _warp(img, ri[0, 0] * x + ri[0, 1] * y + ri[0, 2], ri[1, 0] * x + ri[1, 1] * y + ri[1, 2])
    raise ValueError(name)


def apply_clip(clip, name, M):
    """(T, 3, H, W) -> the same op on every frame."""
    return np.stack([apply_op(fr, name, M) for fr in clip])
