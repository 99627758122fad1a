"""Float64 numpy restatements of the device augmentation (csrc/augment.hip), for
the tests: the photometric chain of the reference's _apply_advanced_augmentation
over a draw_params dict, the flip / rot90 index map, and the noise generator
(Philox4x32-10 + Box-Muller).  Test infrastructure, not product code."""
import numpy as np

STAGES = ("gamma", "contrast", "brightness", "noise_level", "saturation", "shift")


def load_fixture(golden_dir):
    """tests/golden/g9_augment*.npz (make_golden_augment.py) -> (cases, ref_err);
    a case is dict(key, seed, x, noise, out32, out64), arrays [3,H,W]."""
    import os
    index = np.load(os.path.join(golden_dir, "g9_augment.npz"))
    arrays = dict(index)
    for part in index["parts"]:
        arrays.update(np.load(os.path.join(golden_dir, str(part))))
    cases = []
    for key in ("a", "b"):
        for s in arrays[f"{key}_seeds"].tolist():
            cases.append({"key": key, "seed": s, "x": arrays[f"{key}_inputs"][s % 2],
                          "noise": arrays[f"{key}_{s}_noise"], "out32": arrays[f"{key}_{s}_out32"],
                          "out64": arrays[f"{key}_{s}_out64"]})
    return cases, float(arrays["ref_err"])


def chain(x, noise, p):
    """x [3,H,W], noise [3,H,W] (N(0,1) draws), p = draw_params dict -> float64 [3,H,W]."""
    v = np.asarray(x, np.float64)
    if p["gamma"] is not None:
        v = np.power(np.maximum(v, 1e-8), p["gamma"])
    if p["contrast"] is not None:
        m = v.mean(axis=(1, 2), keepdims=True)
        v = np.clip((v - m) * p["contrast"] + m, 0, 1)
    if p["brightness"] is not None:
        v = np.clip(v + p["brightness"], 0, 1)
    if p["noise_level"] is not None:
        v = np.clip(v + np.asarray(noise, np.float64) * p["noise_level"], 0, 1)
    if p["saturation"] is not None:
        gray = 0.299 * v[0] + 0.587 * v[1] + 0.114 * v[2]
        v = np.clip(gray[None] + p["saturation"] * (v - gray[None]), 0, 1)
    if p["shift"] is not None:
        v = np.clip(v + p["shift"], 0, 1)
    return v


def stage_pattern(p):
    return tuple(p[s] is not None for s in STAGES)


def geometry(x, hflip, vflip, k):
    """The inverse index map the kernels use, on a numpy [3,H,W] array:
    even k: out[y][x] = in[fy(y)][fx(x)]; odd k: out[i][j] = in[fy(j)][fx(i)]."""
    _, H, W = x.shape
    if k == 0:
        fy, fx = vflip, hflip
    elif k == 2:
        fy, fx = not vflip, not hflip
    elif k == 1:
        fy, fx = vflip, not hflip
    else:
        fy, fx = not vflip, hflip
    rows = np.arange(H)[::-1] if fy else np.arange(H)
    cols = np.arange(W)[::-1] if fx else np.arange(W)
    src = x[:, rows][:, :, cols]
    return src.transpose(0, 2, 1) if k & 1 else src


M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85


def philox4x32_10(ctr, key):
    """ctr: 4 uint32 arrays (or ints), key: 2 -> 4 uint32 arrays (Random123 philox4x32, 10 rounds)."""
    c = [np.asarray(v, np.uint64) & 0xFFFFFFFF for v in ctr]
    k = [np.uint64(key[0] & 0xFFFFFFFF), np.uint64(key[1] & 0xFFFFFFFF)]
    mask, s32 = np.uint64(0xFFFFFFFF), np.uint64(32)
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]
        c = [(p1 >> s32) ^ c[1] ^ k[0], p1 & mask, (p0 >> s32) ^ c[3] ^ k[1], p0 & mask]
        k = [(k[0] + np.uint64(W0)) & mask, (k[1] + np.uint64(W1)) & mask]
    return [v.astype(np.uint32) for v in c]


def normals(seed, sample_id, Ho, Wo):
    """float64 [3,Ho,Wo]: element idx = (c*Ho + y)*Wo + x takes normal idx % 4
    of counter (sample_id, idx // 4); u = ((r >> 9) + 0.5) 2^-23, the pairs
    (r0, r1) and (r2, r3) give sqrt(-2 ln u1) * (cos, sin)(2 pi u2)."""
    n = 3 * Ho * Wo
    grp = np.arange((n + 3) // 4, dtype=np.uint64)
    zero = np.zeros_like(grp)
    r = philox4x32_10([zero + (sample_id & 0xFFFFFFFF), zero + ((sample_id >> 32) & 0xFFFFFFFF), grp, zero],
                      [seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF])
    u = [((v >> np.uint32(9)).astype(np.float64) + 0.5) / 8388608.0 for v in r]
    ra, rb = np.sqrt(-2.0 * np.log(u[0])), np.sqrt(-2.0 * np.log(u[2]))
    z = np.stack([ra * np.cos(2 * np.pi * u[1]), ra * np.sin(2 * np.pi * u[1]),
                  rb * np.cos(2 * np.pi * u[3]), rb * np.sin(2 * np.pi * u[3])], axis=1)
    return z.reshape(-1)[:n].reshape(3, Ho, Wo)
