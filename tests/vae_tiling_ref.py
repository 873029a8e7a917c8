"""NumPy restatement of diffusers' tiled VAE calls (AutoencoderKL.tiled_decode / tiled_encode, blend_v / blend_h), the SEQUENTIAL
in-place procedure: tiles are blended in row-major order, each against its already blended upper and left neighbours, then cropped and
concatenated.  Written from the specification in include/pdengine.h, not from the engine's closed form; the tests compare the two.

Arithmetic as torch does it on fp32 tensors: the weights 1 - y / e and y / e are Python doubles rounded to fp32 when they meet the
tensor, both products and the sum are fp32 and rounded on their own."""
import numpy as np


def blend_v(a, b, e):
    e = min(a.shape[2], b.shape[2], e)
    for y in range(e):
        b[:, :, y, :] = a[:, :, -e + y, :] * np.float32(1 - y / e) + b[:, :, y, :] * np.float32(y / e)
    return b


def blend_h(a, b, e):
    e = min(a.shape[3], b.shape[3], e)
    for x in range(e):
        b[:, :, :, x] = a[:, :, :, -e + x] * np.float32(1 - x / e) + b[:, :, :, x] * np.float32(x / e)
    return b


def decode_numbers(T, f, u=8):
    """(ov, be, row_limit) of tiled_decode: tile stride in latent pixels, blend extent and kept size in image pixels."""
    return int(T * (1 - f)), int(T * u * f), T * u - int(T * u * f)


def encode_numbers(T, f, u=8):
    """(ov, be, row_limit) of tiled_encode: tile stride in image pixels, blend extent and kept size in latent pixels."""
    return int(T * u * (1 - f)), int(T * f), T - int(T * f)


def is_tiled(h, w, T, u=8, encode=False):
    side = T * u if encode else T
    return h > side or w > side


def windows(h, w, T, f, u=8, encode=False):
    """The grid: rows of (i, j, tile_h, tile_w) in input pixels, as range(0, h, ov) walks it."""
    ov = (encode_numbers if encode else decode_numbers)(T, f, u)[0]
    side = T * u if encode else T
    return [[(i, j, min(side, h - i), min(side, w - j)) for j in range(0, w, ov)] for i in range(0, h, ov)]


def assemble(rows, be, limit):
    """rows: the grid of raw tiles [B, C, th, tw] (fp32); blends them in place, in order, and returns the concatenation of the crops."""
    rows = [[np.array(t, np.float32, copy=True) for t in row] for row in rows]
    result_rows = []
    for i, row in enumerate(rows):
        result_row = []
        for j, tile in enumerate(row):
            if i > 0:
                tile = blend_v(rows[i - 1][j], tile, be)
            if j > 0:
                tile = blend_h(row[j - 1], tile, be)
            result_row.append(tile[:, :, :limit, :limit])
        result_rows.append(np.concatenate(result_row, axis=3))
    return np.concatenate(result_rows, axis=2)


def tiled_decode(z, T, f, fn, u=8):
    """fn: latent tile [B, C, th, tw] -> image tile [B, 3, th u, tw u] (post_quant_conv and decoder)."""
    _, be, limit = decode_numbers(T, f, u)
    rows = [[fn(z[:, :, i:i + th, j:j + tw]) for (i, j, th, tw) in row] for row in windows(z.shape[2], z.shape[3], T, f, u)]
    return assemble(rows, be, limit)


def tiled_encode(x, T, f, fn, u=8):
    """fn: image tile [B, 3, th, tw] -> moments tile [B, 2z, th / u, tw / u] (encoder and quant_conv)."""
    _, be, limit = encode_numbers(T, f, u)
    rows = [[fn(x[:, :, i:i + th, j:j + tw]) for (i, j, th, tw) in row] for row in windows(x.shape[2], x.shape[3], T, f, u, True)]
    return assemble(rows, be, limit)


def plan(h, w, T, f, u=8, encode=False):
    """What pd_vae_tile_plan reports, derived by walking the sequential procedure on shapes alone: a list of rows of dicts."""
    _, be, limit = (encode_numbers if encode else decode_numbers)(T, f, u)
    out = lambda n: n // u if encode else n * u
    grid = []
    for ti, row in enumerate(windows(h, w, T, f, u, encode)):
        grid.append([])
        for tj, (i, j, th, tw) in enumerate(row):
            t = dict(y0=i, x0=j, h=th, w=tw, th=out(th), tw=out(tw), ev=0, eh=0)
            if ti > 0:
                t["ev"] = min(grid[ti - 1][tj]["th"], t["th"], be)
            if tj > 0:
                t["eh"] = min(grid[ti][tj - 1]["tw"], t["tw"], be)
            t["oh"], t["ow"] = min(limit, t["th"]), min(limit, t["tw"])
            t["oy"] = sum(grid[k][tj]["oh"] for k in range(ti))
            t["ox"] = sum(grid[ti][k]["ow"] for k in range(tj))
            grid[ti].append(t)
    return grid
