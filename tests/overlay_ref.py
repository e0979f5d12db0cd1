"""The diff image of include/twflow.h ("Diff image"), in plain numpy, written from the header's text and from nothing else.

overlay_ref(E, T, rects, hits, boxes, tol) -> (h, w, 3) uint8.  rects: the pair's CLIPPED ignore rectangles (x, y, width,
height); hits: (x, y, dx, dy) with dx, dy as the float32 values the engine holds, already after the ignore rule; boxes: (x, y,
width, height, ...) region records.  clip_rects() is the submit's clipping, outside() the ignore rule."""
import numpy as np

MAX_LEN = 1024
BOX_RGB = (0, 160, 0)
VEC_RGB = (0, 0, 255)


def clip_rects(rects, w, h):
    """Each rectangle clipped to the w x h image, the empty ones dropped."""
    out = []
    for x, y, rw, rh in rects:
        x0, y0, x1, y1 = max(x, 0), max(y, 0), min(x + rw, w), min(y + rh, h)
        if x1 > x0 and y1 > y0:
            out.append((x0, y0, x1 - x0, y1 - y0))
    return out


def inside(rects, x, y):
    return any(rx <= x < rx + rw and ry <= y < ry + rh for rx, ry, rw, rh in rects)


def outside(hits, rects):
    """The ignore rule: the hits whose grid point lies in no clipped rectangle."""
    return [h for h in hits if not inside(rects, h[0], h[1])]


def q(v):
    """0 when v is NaN, else (int) round-half-even of min(max(v, -1024.f), 1024.f)."""
    v = np.float32(v)
    if np.isnan(v):
        return 0
    v = min(max(v, np.float32(-MAX_LEN)), np.float32(MAX_LEN))
    return int(np.rint(v))  # numpy's rint rounds half to even


def line_pixels(x, y, dx, dy):
    """The marker's and the line's pixels of one hit, before the drop of those outside the image."""
    rx, ry = q(dx), q(dy)
    n = max(abs(rx), abs(ry))
    px = [(x + i, y + j) for j in (-1, 0, 1) for i in (-1, 0, 1)]
    if n == 0:
        px.append((x, y))
    else:
        for i in range(n + 1):
            # Python's // is floor division
            px.append((x + (2 * i * rx + n) // (2 * n), y + (2 * i * ry + n) // (2 * n)))
    return px


def box_pixels(x, y, bw, bh):
    if bw < 1 or bh < 1:
        return []
    px = [(x + i, y) for i in range(bw)] + [(x + i, y + bh - 1) for i in range(bw)]
    px += [(x, y + j) for j in range(bh)] + [(x + bw - 1, y + j) for j in range(bh)]
    return px


def base_ref(E, T, rects, tol):
    E = np.asarray(E, np.uint8).astype(np.int32)
    T = np.asarray(T, np.uint8).astype(np.int32)
    h, w = E.shape
    d = np.abs(E - T)
    g = 128 + (T >> 1)
    img = np.stack([g, g, g], axis=-1)
    ch = d > tol
    img[ch] = np.stack([np.full_like(d, 255), 192 - (d >> 1), np.zeros_like(d)], axis=-1)[ch]
    m = np.zeros((h, w), bool)
    for x, y, rw, rh in rects:
        m[max(y, 0):max(y + rh, 0), max(x, 0):max(x + rw, 0)] = True
    img[m] = np.stack([g - 48, g - 48, g], axis=-1)[m]
    assert img.min() >= 0 and img.max() <= 255
    return img.astype(np.uint8)


def overlay_ref(E, T, rects, hits, boxes, tol):
    img = base_ref(E, T, rects, tol)
    h, w = img.shape[:2]

    def put(pixels, rgb):
        for x, y in pixels:
            if 0 <= x < w and 0 <= y < h:
                img[y, x] = rgb

    for b in boxes:
        put(box_pixels(int(b[0]), int(b[1]), int(b[2]), int(b[3])), BOX_RGB)
    for x, y, dx, dy in hits:
        put(line_pixels(int(x), int(y), dx, dy), VEC_RGB)
    return img
