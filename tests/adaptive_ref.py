"""numpy references of the second moments, the tile noise estimate and the adaptive driver
(include/pt_hip.h: pt_render_moments, pt_noise_tiles_async, pt_tile_mean_async, pt_render_adaptive),
shared by test_gpu_moments.py, test_gpu_adaptive.py and test_adaptive_cpu.py.  Every operation is
rounded once and in the order the header states, so the library's results are compared bit for bit."""
import numpy as np

TILE_NOISE_DTYPE = np.dtype([("noisy", "<u4"), ("pixels", "<u4"), ("max_err", "<f8")])


def moments(frames, acc=None, m2=None):
    """acc += c and m2 = m2 + c * c over `frames` (raw radiance [h, w, 3] f32 each, in frame order),
    c = clamp(L): f32 throughout, the product rounded before the sum."""
    frames = list(frames)
    shape = frames[0].shape
    acc = np.zeros(shape, np.float32) if acc is None else np.array(acc, np.float32)
    m2 = np.zeros(shape, np.float32) if m2 is None else np.array(m2, np.float32)
    for L in frames:
        c = np.where(L >= 0, L, 0).astype(np.float32)
        acc = acc + c
        m2 = m2 + c * c
    assert acc.dtype == np.float32 and m2.dtype == np.float32
    return acc, m2


def tile_grid(w, h, tile):
    tw, th = tile
    return -(-w // tw), -(-h // th)


def frames_of_pixels(frames, w, h, tile):
    """The [h, w] sample counts of the pixels from the tiles' [TY, TX]."""
    tw, th = tile
    f = np.asarray(frames)
    return np.repeat(np.repeat(f, th, axis=0), tw, axis=1)[:h, :w]


def pixel_err(acc, m2, n, floor):
    """err of every pixel, float64, n [h, w] >= 2 (other n: garbage the caller overrides)."""
    S, Q = np.asarray(acc, np.float32).astype(np.float64), np.asarray(m2, np.float32).astype(np.float64)
    n = np.asarray(n, np.float64)
    with np.errstate(all="ignore"):
        d = Q - (S * S) / n[..., None]
        v = np.where(d > 0, d, 0.0)
        V = (v[..., 0] + v[..., 1]) + v[..., 2]
        se = np.sqrt(V / (n * (n - 1)))
        mu = ((S[..., 0] + S[..., 1]) + S[..., 2]) / n
        den = np.where(mu > floor, mu, floor)
        return se / den


def noise_tiles(acc, m2, tile, frames, tol, floor):
    """pt_noise_tiles in numpy: [TY, TX] of TILE_NOISE_DTYPE."""
    h, w = acc.shape[:2]
    tw, th = tile
    tx, ty = tile_grid(w, h, tile)
    frames = np.asarray(frames, np.uint32).reshape(ty, tx)
    err = pixel_err(acc, m2, frames_of_pixels(frames, w, h, tile), floor)
    out = np.zeros((ty, tx), TILE_NOISE_DTYPE)
    for j in range(ty):
        for i in range(tx):
            e = err[j * th:(j + 1) * th, i * tw:(i + 1) * tw]
            out[j, i]["pixels"] = e.size
            if frames[j, i] < 2:
                out[j, i]["noisy"], out[j, i]["max_err"] = e.size, np.inf
                continue
            with np.errstate(invalid="ignore"):
                out[j, i]["noisy"] = int(np.count_nonzero(e > tol))
            m = 0.0  # the running (err > m ? err : m): a NaN never enters
            for x in e.ravel():
                m = x if x > m else m
            out[j, i]["max_err"] = m
    return out


def tile_mean(acc, tile, frames):
    h, w = acc.shape[:2]
    n = frames_of_pixels(frames, w, h, tile).astype(np.float32)[..., None]
    with np.errstate(all="ignore"):
        return np.where(n > 0, np.asarray(acc, np.float32) / n, np.float32(0)).astype(np.float32)


def tile_rects(active):
    """The rectangles (tx0, ty0, width, height) of a [TY, TX] mask: rows top to bottom, maximal runs;
    a run with the columns of a rectangle that reached the row above extends it."""
    a = np.asarray(active) != 0
    rects, prev = [], {}
    for y in range(a.shape[0]):
        cur, x = {}, 0
        while x < a.shape[1]:
            if not a[y, x]:
                x += 1
                continue
            x1 = x
            while x1 < a.shape[1] and a[y, x1]:
                x1 += 1
            k = prev.get((x, x1))
            if k is None:
                k = len(rects)
                rects.append([x, y, x1 - x, 1])
            else:
                rects[k][3] += 1
            cur[(x, x1)] = k
            x = x1
        prev = cur
    return np.array(rects, np.uint32).reshape(-1, 4)


def simulate(frame_fn, w, h, tile, frame0, min_frames, step_frames, max_frames, tol, floor, noisy_fraction):
    """pt_render_adaptive over frame_fn(k) -> the window's raw radiance [h, w, 3] of frame k: pass 0,
    verdicts, active set, next frame range, ...  Returns accum, m2, tile_frames, tile_noise, passes
    and the rectangles of every refinement pass."""
    tw, th = tile
    tx, ty = tile_grid(w, h, tile)
    acc, m2 = moments([frame_fn(frame0 + k) for k in range(min_frames)])
    frames = np.full((ty, tx), min_frames, np.uint32)
    done, passes, rect_log = min_frames, 1, []
    while True:
        noise = noise_tiles(acc, m2, tile, frames, tol, floor)
        limit = (noisy_fraction * noise["pixels"].astype(np.float64)).astype(np.uint32)
        active = (noise["noisy"] > limit) & (frames < max_frames)
        if not active.any():
            break
        nf = min(step_frames, max_frames - done)
        new = [frame_fn(frame0 + done + k) for k in range(nf)]
        rects = tile_rects(active)
        rect_log.append(rects)
        for rx, ry, rw, rh in rects.astype(int):
            ys, xs = slice(ry * th, min((ry + rh) * th, h)), slice(rx * tw, min((rx + rw) * tw, w))
            acc[ys, xs], m2[ys, xs] = moments([L[ys, xs] for L in new], acc[ys, xs], m2[ys, xs])
        frames[active] += nf
        done += nf
        passes += 1
    return {"accum": acc, "m2": m2, "tile_frames": frames, "tile_noise": noise, "passes": passes, "rects": rect_log}
