"""numpy restatement of GridMapCvConverter::addLayerFromImage<Type, N> as include/travgpu.h states it: float32 operations one
at a time, integer grey values.  What te_upload_image is compared against, bit for bit."""
import numpy as np

GREY_WEIGHTS = (3735, 19235, 9798)  # applied to the first three channels in memory order; they sum to 1 << GREY_SHIFT
GREY_SHIFT = 15


def samples_from_bytes(data, height, width, step, channels, bytes_per_channel, is_bigendian):
    """The height x width x channels sample values of an image given as raw bytes with row pitch `step`."""
    raw = np.frombuffer(bytes(data), np.uint8)
    row = width * channels * bytes_per_channel
    idx = (np.arange(height) * step)[:, None] + np.arange(row)[None, :]
    b = raw[idx].reshape(height, width, channels, bytes_per_channel).astype(np.uint32)
    if bytes_per_channel == 1:
        return b[..., 0].astype(np.uint8)
    hi, lo = (b[..., 0], b[..., 1]) if is_bigendian else (b[..., 1], b[..., 0])
    return ((hi << 8) | lo).astype(np.uint16)


def alpha_threshold_sample(alpha_threshold, dtype):
    """thr = (T)(alpha_threshold * maxv), truncated; maxv = (float)numeric_limits<T>::max()."""
    return int(float(alpha_threshold) * float(np.float32(np.iinfo(dtype).max)))


def grey(c0, c1, c2):
    c0, c1, c2 = (np.asarray(c, dtype=np.uint64) for c in (c0, c1, c2))
    return (c0 * GREY_WEIGHTS[0] + c1 * GREY_WEIGHTS[1] + c2 * GREY_WEIGHTS[2] + (1 << (GREY_SHIFT - 1))) >> GREY_SHIFT


def add_layer_from_image(samples, lower, upper, alpha_threshold=0.5):
    """samples: H x W or H x W x C (C = 1, 3, 4) of uint8 / uint16 -> the H x W float32 layer (NaN where alpha < thr)."""
    s = np.asarray(samples)
    assert s.dtype in (np.uint8, np.uint16), s.dtype
    if s.ndim == 2:
        s = s[:, :, None]
    ch = s.shape[2]
    assert ch in (1, 3, 4), ch
    g = s[..., 0].astype(np.uint64) if ch == 1 else grey(s[..., 0], s[..., 1], s[..., 2])
    maxv = np.float32(np.iinfo(s.dtype).max)
    lower, upper = np.float32(lower), np.float32(upper)
    q = g.astype(np.float32) / maxv          # (float)g / maxv
    rng = np.float32(upper - lower)          # upper - lower
    prod = (rng * q).astype(np.float32)      # one rounding
    v = (lower + prod).astype(np.float32)    # one rounding
    if ch == 4:
        v = np.where(s[..., 3] < alpha_threshold_sample(alpha_threshold, s.dtype), np.float32(np.nan), v).astype(np.float32)
    return v


def layer_order(v):
    """An H x W layer as te_download_layer returns it: column-major, element (i, j) at j * H + i."""
    return np.ascontiguousarray(np.asarray(v, np.float32).T).reshape(-1)
