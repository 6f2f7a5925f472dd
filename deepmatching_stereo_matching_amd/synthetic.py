"""Synthetic stereo pairs ("Synthetic generator").

The reference ships no data (``.gitignore:2-3`` ignores ``data/``), so every benchmark and
most parity cases use Gaussian-smoothed uniform texture with a known horizontal shift.
Pure numpy (separable Gaussian, sigma=1.0, truncate=4.0 like scipy's default) so the
generator runs identically here and on the GPU box.
"""

import numpy as np


def _gauss_kernel(sigma=1.0, truncate=4.0):
    r = int(truncate * sigma + 0.5)
    x = np.arange(-r, r + 1, dtype=np.float64)
    k = np.exp(-0.5 * (x / sigma) ** 2)
    return k / k.sum()


def _smooth(a, sigma=1.0):
    k = _gauss_kernel(sigma)
    r = len(k) // 2
    out = a.astype(np.float64)
    for axis in (0, 1):
        pad = [(0, 0), (0, 0)]
        pad[axis] = (r, r)
        p = np.pad(out, pad, mode='reflect')
        acc = np.zeros_like(out)
        for t in range(len(k)):
            sl = [slice(None), slice(None)]
            sl[axis] = slice(t, t + out.shape[axis])
            acc += k[t] * p[tuple(sl)]
        out = acc
    return out


def texture(h, w, seed, sigma=1.0):
    """uint8 texture of shape (h, w): uniform noise, smoothed, stretched to [0, 255]."""
    rng = np.random.default_rng(seed)
    raw = rng.integers(0, 256, size=(h, w)).astype(np.float64)
    s = _smooth(raw, sigma)
    lo, hi = s.min(), s.max()
    return np.rint((s - lo) * (255.0 / (hi - lo))).astype(np.uint8)


def stereo_pair(h, w, seed=0, dx=2, max_disp=None, sinusoidal=False):
    """Return (img1, img2), uint8 (h, w): img2 is img1's texture shifted by dx columns.

    With ``sinusoidal=True`` the shift varies smoothly in [0, max_disp] across the image
    (the "realism" runs of SURVEY.md section 8d)."""
    if max_disp is None:
        max_disp = max(dx, 8)
    tex = texture(h + 8, w + 8 + max_disp, seed)
    img1 = tex[4:4 + h, 4:4 + w].copy()
    if not sinusoidal:
        img2 = tex[4:4 + h, 4 + dx:4 + dx + w].copy()
    else:
        yy, xx = np.mgrid[0:h, 0:w]
        d = np.rint(0.5 * max_disp * (1.0 + np.sin(2 * np.pi * xx / max(w, 1)) *
                                      np.cos(2 * np.pi * yy / max(h, 1)))).astype(np.int64)
        img2 = tex[4 + yy, 4 + xx + d].astype(np.uint8)
    return img1, img2


def subpixel_pair(h, w, seed, ky, kx, up=4):
    """Return (img1, img2), uint8 (h, w), with a known sub-pixel shift: the texture is generated
    at ``up`` times the resolution with sigma = up, img1 is every up-th pixel of it from phase
    (0, 0) and img2 every up-th pixel from phase (ky, kx), 0 <= ky, kx < up.  So img2(y, x) =
    img1(y + ky / up, x + kx / up): the match of img1's pixel lies ky / up rows and kx / up columns
    before it, and the true d_map is +ky / up in 'elevation2' and +kx / up in 'elevation'."""
    if not (0 <= ky < up and 0 <= kx < up):
        raise ValueError('the phase (ky, kx) must lie in [0, up)')
    tex = texture(up * (h + 1), up * (w + 1), seed, sigma=float(up))
    img1 = tex[0:up * h:up, 0:up * w:up].copy()
    img2 = tex[ky:ky + up * h:up, kx:kx + up * w:up].copy()
    return img1, img2


def _noisy(img, rng, noise):
    """img plus one draw of Gaussian noise of its shape, rounded and clipped to uint8."""
    return np.clip(np.rint(img.astype(np.float64) + rng.normal(0.0, noise, img.shape)), 0, 255).astype(np.uint8)


def weak_pair(h, w, seed, block, contrast=1.0 / 16, noise=6.0, dx=2):
    """Return (img1, img2), uint8 (h, w): stereo_pair's texture shifted by dx columns (the true d_map
    is 0 in 'elevation2' and dx in 'elevation'), with a weakly textured region under sensor noise.
    ``block`` = (y0, y1, x0, x1): in the rows y0 .. y1-1 and columns x0 .. x1-1 of img1 -- and so dx
    columns to the left of them in img2 -- the texture's deviation from the mean of the whole
    texture is multiplied by ``contrast`` before it is rounded.  Then Gaussian noise of sigma
    ``noise`` is added to both images, rounded and clipped.  The random draws, in this order:
    texture(h + 8, w + 8 + dx, seed) with its own generator; then from default_rng([seed, 1]) one
    normal draw of shape (h, w) for img1, then one for img2."""
    y0, y1, x0, x1 = block
    tex = texture(h + 8, w + 8 + dx, seed).astype(np.float64)
    mean = tex.mean()
    tex[4 + y0:4 + y1, 4 + x0:4 + x1] = mean + (tex[4 + y0:4 + y1, 4 + x0:4 + x1] - mean) * contrast
    tex = np.rint(tex)
    rng = np.random.default_rng([seed, 1])
    img1 = _noisy(tex[4:4 + h, 4:4 + w], rng, noise)
    img2 = _noisy(tex[4:4 + h, 4 + dx:4 + dx + w], rng, noise)
    return img1, img2


def step_pair(h, w, seed, xc, d_left=1, d_right=4, noise=6.0):
    """Return (img1, img2), uint8 (h, w), with a disparity step at column xc: img2's column x' shows
    the texture of img1's column x' + d_left for x' < xc and of column x' + d_right for x' >= xc,
    d_right > d_left.  So img1's columns x < xc + d_left have the disparity d_left and its columns
    x >= xc + d_right the disparity d_right ('elevation'; 'elevation2' is 0); the columns between
    them are seen nowhere in img2 (the step's occlusion).  Then Gaussian noise of sigma ``noise`` is
    added to both images, rounded and clipped.  The random draws, in this order:
    texture(h + 8, w + 8 + d_right, seed) with its own generator; then from default_rng([seed, 2])
    one normal draw of shape (h, w) for img1, then one for img2."""
    if not d_right > d_left >= 0:
        raise ValueError('step_pair needs 0 <= d_left < d_right')
    tex = texture(h + 8, w + 8 + d_right, seed)
    xx = np.arange(w)
    src = np.where(xx < xc, xx + d_left, xx + d_right)
    rng = np.random.default_rng([seed, 2])
    img1 = _noisy(tex[4:4 + h, 4:4 + w], rng, noise)
    img2 = _noisy(tex[4:4 + h, 4 + src], rng, noise)
    return img1, img2


CONTENT_KINDS = ('binary', 'identical', 'dark', 'bright', 'dark_bright', 'low4', 'high4',
                 'checker', 'stripes', 'edge', 'const')


def content_pair(kind, h, w, seed):
    """Return (img1, img2), uint8 (h, w), of one content class of CONTENT_KINDS: images at the
    ends of the value range, with exact ties, or flat -- what the smooth texture of stereo_pair
    never is ("Value ranges").  Unless noted below, a field of w + 3
    columns is generated and img1 = field[:, :w], img2 = field[:, 3:] (a shift of 3 columns).

      binary       i.i.d. pixels in {0, 255}
      identical    binary, img2 == img1 (r = 1 exactly at q = p)
      dark         0, and 255 with probability 0.02: flat patches next to textured ones at
                   ws = 5, and still an all-zero 15 x 15 patch in a tile (the lowest sums)
      bright       255 - dark
      dark_bright  dark against 255 - its shifted self (the most negative products)
      low4         i.i.d. pixels in {0 .. 3}
      high4        252 + low4 (tiny variances under the largest sums)
      checker      255 * ((x // 2 + y // 2) % 2), img2 shifted by 1 column (every row of
                   level 0 has many exact maxima)
      stripes      10 where x % 8 < 4, else 240
      edge         0 left of column w // 2 of the field, 255 from there on
      const        img1 all 255, img2 all 0 (every patch and every window flat)"""
    if kind not in CONTENT_KINDS:
        raise ValueError('unknown content kind %r' % (kind,))
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w + 3]
    if kind in ('binary', 'identical'):
        f = 255 * rng.integers(0, 2, size=(h, w + 3))
    elif kind in ('dark', 'bright', 'dark_bright'):
        f = 255 * (rng.random((h, w + 3)) < 0.02)
        if kind == 'bright':
            f = 255 - f
    elif kind in ('low4', 'high4'):
        f = rng.integers(0, 4, size=(h, w + 3)) + (252 if kind == 'high4' else 0)
    elif kind == 'checker':
        f = 255 * ((xx // 2 + yy // 2) % 2)
    elif kind == 'stripes':
        f = np.where(xx % 8 < 4, 10, 240)
    elif kind == 'edge':
        f = np.where(xx < w // 2, 0, 255)
    else:
        f = np.full((h, w + 3), 255)
    f = f.astype(np.uint8)
    img1 = f[:, :w].copy()
    if kind == 'identical':
        img2 = img1.copy()
    elif kind == 'dark_bright':
        img2 = 255 - f[:, 3:]
    elif kind == 'checker':
        img2 = f[:, 1:w + 1].copy()
    elif kind == 'const':
        img2 = np.zeros((h, w), dtype=np.uint8)
    else:
        img2 = f[:, 3:].copy()
    return img1, img2


def ramp_pair(h, w, seed, g, axis=1, d0=2.0, up=8, noise=0.0):
    """Return (img1, img2, d), uint8 (h, w) twice and float64 (h, w): a pair whose disparity is a
    linear ramp of slope ``g`` along the columns (a slope of the terrain), and the true disparity.
    The texture is generated at ``up`` times the resolution with sigma = up; img1 is every up-th
    pixel of it; img2(y, x) is the texture at the column x + d0 + g (x - w / 2), interpolated
    linearly between the two nearest pixels of the fine grid and rounded.  The texture is padded on
    both sides so that no index leaves it.  img1's column x1 is seen in img2 at x2 = (x1 - d0 +
    g w / 2) / (1 + g), so the true d_map is d = x1 - x2 in 'elevation' and 0 in 'elevation2', and
    the matched window is stretched by dx2/dx1 = 1 / (1 + g).  ``axis=0`` builds the pair of (w, h)
    and transposes it: the ramp runs along the rows, d belongs to 'elevation2' and 'elevation' is 0.
    With ``noise`` > 0 Gaussian noise of that sigma is added to both images, rounded and clipped.
    The random draws, in this order: texture(up h, up (w + pad), seed, sigma=up) with its own
    generator; then, with noise, from default_rng([seed, 3]) one normal draw of shape (h, w) for
    img1, then one for img2 (before the transposition of axis=0)."""
    if axis == 0:
        a, b, d = ramp_pair(w, h, seed, g, 1, d0, up, noise)
        return a.T.copy(), b.T.copy(), d.T.copy()
    if axis != 1:
        raise ValueError('axis must be 0 or 1')
    if not g > -1.0:
        raise ValueError('ramp_pair needs a slope g > -1')
    xx = np.arange(w, dtype=np.float64)
    s = d0 + g * (xx - w / 2.0)
    left, right = int(np.ceil(max(0.0, -s.min()))) + 1, int(np.ceil(max(0.0, s.max()))) + 2
    tex = texture(up * h, up * (w + left + right), seed, sigma=float(up))[0:up * h:up].astype(np.float64)
    img1 = tex[:, up * left:up * (left + w):up]
    pos = up * (left + xx + s)
    i0 = np.floor(pos).astype(np.int64)
    f = pos - i0
    img2 = np.rint((1.0 - f) * tex[:, i0] + f * tex[:, i0 + 1])
    if noise > 0:
        rng = np.random.default_rng([seed, 3])
        img1, img2 = _noisy(img1, rng, noise), _noisy(img2, rng, noise)
    d = xx - (xx - d0 + g * w / 2.0) / (1.0 + g)
    return img1.astype(np.uint8), img2.astype(np.uint8), np.tile(d, (h, 1))
