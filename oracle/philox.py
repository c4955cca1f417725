"""Host restatement of the production noise path: Philox4x32-10 and every draw site of the HIP kernels (numpy, CPU only).

Written from the published algorithm (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11) and from
`stylesinger_amd/csrc/common.h` (`SsPhilox`, `ss_u01`, `ss_boxmuller`, `ss_mel_draw4`). The generator is pinned by the Random123 known-answer
vectors (tests/test_noise_cpu.py); the kernels are pinned to this file (tests/test_gpu_noise.py).

A draw site is a kernel that turns a counter block into noise. Every site has ONE counter function here (`ctr_*`: index -> (c0, c1, c2, c3) as
unbounded integers, i.e. before the kernel's casts to uint32_t), used both to draw the site's tensor and to analyse which blocks a run touches
(`run_blocks`). The key of a launch is `host key + seed` modulo 2^64 (`seed + *seed_dev` in the kernels); the host keys are the constants
`StyleSingerHIP` passes (KEY_*).

    site                  kernel                                  counter (c0, c1, c2, c3)                       words used
    fill_normal           fill_normal_kernel                      (lo(off + i), hi(off + i), 'FILL', 0)          all four: values 4 i .. 4 i + 3
    fill_normal_rows      fill_normal_rows_kernel                 (t / 4, b, 'FILL', 1)                          all four: frames 4 (t / 4) .. + 3
    mel_qsample           mel_qsample_kernel                      (t * M + c, b, 0xffffffff, 'MELD')             z0 only
    mel_step              SS_EPI_DDPM epilogue, mel_tail_kernel   ((t >> 2) * N + n, b, step, 'MELD')            all four: output t & 3
    f0_step               f0_update_row                           (t, b, step, 'F0UV')                           z0 ; u0 = o[2], u1 = o[3] in [0, 1)
    rand_ini              src_base_kernel                         (b * NH + h, 0, 'RINI', 'NSF1'), h > 0         o[0] in [0, 1)
    sine_noise            src_final_kernel                        (lo(ctr), hi(ctr), 'SINE', 'NSF2')             z0 only ; ctr = (b * L + i) * NH + h

`step` is the NETWORK TIME t of the update in every sampler (ddpm, ddim at any stride, ProDiff), not a loop index.
"""
import math

import numpy as np

M32 = 0xFFFFFFFF
M64 = 0xFFFFFFFFFFFFFFFF
PHILOX_M0, PHILOX_M1 = 0xD2511F53, 0xCD9E8D57
PHILOX_W0, PHILOX_W1 = 0x9E3779B9, 0xBB67AE85

TAG_FILL, TAG_MELD, TAG_F0UV = 0x46494C4C, 0x4D454C44, 0x46305556
TAG_RINI, TAG_NSF1, TAG_SINE, TAG_NSF2 = 0x52494E49, 0x4E534631, 0x53494E45, 0x4E534632
QSAMPLE_STEP = 0xFFFFFFFF

# host parts of the keys (stylesinger_amd/model.py): f0 x_T, f0 steps, mel q-sample, mel steps of the batch half that starts at item b0,
# ddim steps / ProDiff x_T, ProDiff steps
KEY_F0_Z0, KEY_F0_STEPS, KEY_MEL_Q, KEY_MEL_STEPS, KEY_MEL_ALT, KEY_PRODIFF_STEPS = 11, 17, 23, 29, 31, 37
KEY_HALF_STRIDE = 7919


def key_mel_steps(b0):
    return KEY_MEL_STEPS + KEY_HALF_STRIDE * int(b0)


def make_key(host_key, seed=0, seed_dev=0):
    """`seed + *seed_dev` of the kernels with seed = host key + the caller's host seed: 64-bit wrap-around addition."""
    return (int(host_key) + int(seed) + int(seed_dev)) & M64


# ------------------------------------------------------------------------------------------------
# generator and transforms
# ------------------------------------------------------------------------------------------------
def philox4x32_10(c0, c1, c2, c3, key64):
    """Philox4x32 with 10 rounds, vectorised over the counter words (anything numpy broadcasts; values < 2^32) -> four uint32 arrays."""
    c = [np.asarray(x, dtype=np.uint64) for x in (c0, c1, c2, c3)]
    for x in c:
        assert x.size == 0 or int(x.max()) <= M32, "counter word exceeds 32 bits"
    c0, c1, c2, c3 = np.broadcast_arrays(*c)
    key64 = int(key64) & M64
    k0, k1 = key64 & M32, key64 >> 32
    m32, s32 = np.uint64(M32), np.uint64(32)
    for _ in range(10):
        p0 = np.uint64(PHILOX_M0) * c0      # 32 x 32 -> 64 bits: exact in uint64
        p1 = np.uint64(PHILOX_M1) * c2
        hi0, lo0, hi1, lo1 = p0 >> s32, p0 & m32, p1 >> s32, p1 & m32
        c0, c1, c2, c3 = hi1 ^ c1 ^ np.uint64(k0), lo1, hi0 ^ c3 ^ np.uint64(k1), lo0
        k0, k1 = (k0 + PHILOX_W0) & M32, (k1 + PHILOX_W1) & M32
    return tuple(x.astype(np.uint32) for x in (c0, c1, c2, c3))


def u01(word):
    """ss_u01: 32-bit word -> uniform in (0, 1], exact in fp32 and here."""
    return ((np.asarray(word, dtype=np.uint64) >> np.uint64(8)).astype(np.float64) + 1.0) * 2.0 ** -24


def u_open(word):
    """The [0, 1) form of the Gumbel and rand_ini draws (like torch.rand): exact in fp32 and here."""
    return (np.asarray(word, dtype=np.uint64) >> np.uint64(8)).astype(np.float64) * 2.0 ** -24


def radius(a):
    """Box-Muller radius sqrt(-2 ln u1) of word a (float64): <= sqrt(48 ln 2) = 5.768..."""
    return np.sqrt(-2.0 * np.log(u01(a)))


def boxmuller(a, b):
    """ss_boxmuller in float64 from the exact uniforms: words (a, b) -> (z0, z1) = r (cos, sin)(2 pi u2)."""
    r, th = radius(a), 2.0 * math.pi * u01(b)
    return r * np.cos(th), r * np.sin(th)


def normal_bound(r):
    """Per-element bound on |z_device - z_host| for a draw of radius r: the fp32 angle fl(2 pi) u2 is off by at most |fl(2 pi) - 2 pi| u2 +
    ulp(theta) / 2 <= 1.8e-7 + 2.4e-7, which moves z by at most r * 4.2e-7 < r 2^-21; a few ulp of logf / sincosf / the product make the + 1."""
    return (np.asarray(r, dtype=np.float64) + 1.0) * 2.0 ** -21


def _four_normals(o):
    """a block's four words -> [4, ...] normals (two Box-Muller pairs, the order of the kernels) and their radii"""
    z0, z1 = boxmuller(o[0], o[1])
    z2, z3 = boxmuller(o[2], o[3])
    r01, r23 = radius(o[0]), radius(o[2])
    return np.stack([z0, z1, z2, z3]), np.stack([r01, r01, r23, r23])


# ------------------------------------------------------------------------------------------------
# counter layouts: index -> (c0, c1, c2, c3) BEFORE the kernels' casts to uint32_t (Python ints or integer arrays)
# ------------------------------------------------------------------------------------------------
def ctr_fill_normal(i, offset=0):
    c = (offset + i) & M64
    return c & M32, c >> 32, TAG_FILL, 0


def ctr_fill_normal_rows(t4, b):
    return t4, b, TAG_FILL, 1


def ctr_mel_qsample(t, c, b, M):
    return t * M + c, b, QSAMPLE_STEP, TAG_MELD


def ctr_mel_step(t4, n, b, step, N):
    return t4 * N + n, b, step, TAG_MELD


def ctr_f0_step(t, b, step):
    return t, b, step, TAG_F0UV


def ctr_rand_ini(b, h, NH):
    return b * NH + h, 0, TAG_RINI, TAG_NSF1


def ctr_sine_noise(b, i, h, L, NH):
    c = (b * L + i) * NH + h
    return c & M32, c >> 32, TAG_SINE, TAG_NSF2


def _idx(*shape):
    """open index grids as uint64 (ogrid)"""
    return [np.arange(n, dtype=np.uint64).reshape([-1 if k == j else 1 for k in range(len(shape))]) for j, n in enumerate(shape)]


def _ret(z, r, want_radius):
    return (z, r) if want_radius else z


# ------------------------------------------------------------------------------------------------
# draw sites: the site's whole tensor in float64 (with want_radius: also the Box-Muller radius of every element, for normal_bound)
# ------------------------------------------------------------------------------------------------
def fill_normal(n, key, offset=0, want_radius=False):
    """ss_fill_normal: x[0 .. n) ; block i holds values 4 i .. 4 i + 3."""
    nb = (n + 3) // 4
    c0, c1, c2, c3 = ctr_fill_normal(np.arange(nb, dtype=object), int(offset))     # Python integers: the 64-bit sum wraps like the kernel's
    c0, c1 = c0.astype(np.uint64), c1.astype(np.uint64)
    z, r = _four_normals(philox4x32_10(c0, c1, c2, c3, key))
    return _ret(z.T.reshape(-1)[:n], r.T.reshape(-1)[:n], want_radius)


def fill_normal_rows(B, T, key, want_radius=False):
    """ss_fill_normal_rows: [B, T]; the first T' <= T columns do not depend on T."""
    b, t4 = _idx(B, (T + 3) // 4)
    z, r = _four_normals(philox4x32_10(*ctr_fill_normal_rows(t4, b), key))          # [4, B, T/4]
    f = lambda a: np.moveaxis(a, 0, -1).reshape(B, -1)[:, :T]
    return _ret(f(z), f(r), want_radius)


def mel_qsample_noise(B, T, M, key, want_radius=False):
    """ss_mel_qsample: [B, T, M], one block per element, z0 of the block."""
    b, t, c = _idx(B, T, M)
    o = philox4x32_10(*ctr_mel_qsample(t, c, b, np.uint64(M)), key)
    return _ret(boxmuller(o[0], o[1])[0], radius(o[0]), want_radius)


def mel_step_noise(B, T, N, step, key, want_radius=False):
    """The mel sampler's draw at network time `step` (ss_mel_draw4): [B, T, N]; element (b, t, n) = output t & 3 of block ((t >> 2) N + n, b, step)."""
    b, t4, n = _idx(B, (T + 3) // 4, N)
    z, r = _four_normals(philox4x32_10(*ctr_mel_step(t4, n, b, int(step), np.uint64(N)), key))   # [4, B, T/4, N]
    f = lambda a: np.moveaxis(a, 0, 2).reshape(B, -1, N)[:, :T]
    return _ret(f(z), f(r), want_radius)


def f0_step_draws(B, T, step, key, want_radius=False):
    """f0_update_row at network time `step`: (z [B, T], u [B, 2, T]) - the Gaussian draw and the two Gumbel uniforms in [0, 1)."""
    b, t = _idx(B, T)
    o = philox4x32_10(*ctr_f0_step(t, b, int(step)), key)
    z = boxmuller(o[0], o[1])[0]
    u = np.stack([u_open(o[2]), u_open(o[3])], axis=1)
    return (z, u, radius(o[0])) if want_radius else (z, u)


def rand_ini(B, key, NH=9):
    """src_base_kernel: [B, NH] initial phases in [0, 1); harmonic 0 (the fundamental) starts at 0 and draws nothing."""
    b, h = _idx(B, NH)
    u = u_open(philox4x32_10(*ctr_rand_ini(b, h, np.uint64(NH)), key)[0])
    u[:, 0] = 0.0
    return u


def sine_noise(B, L, key, NH=9, want_radius=False):
    """src_final_kernel: [B, L, NH], one block per element (64-bit counter), z0 of the block."""
    b, i, h = _idx(B, L, NH)
    assert B * L * NH < 2 ** 63
    o = philox4x32_10(*ctr_sine_noise(b, i, h, np.uint64(L), np.uint64(NH)), key)
    return _ret(boxmuller(o[0], o[1])[0], radius(o[0]), want_radius)


# ------------------------------------------------------------------------------------------------
# whole models
# ------------------------------------------------------------------------------------------------
def model_noise(seed, B, T, steps_f0, steps_mel, bounds=None, M=80, want_radius=False):
    """What `StyleSingerHIP.forward(..., seed=seed)` draws on the device (default ancestral sampler), as the dict `synth.draw_acoustic_noise`
    returns (reference layouts, float64 torch tensors): f0_a / f0_b: z0 [B,1,T], z_steps [S,B,1,T], u_steps [S,B,2,T], u_init (unused by both
    paths: zeros); mel: z_q [B,1,M,T], z_steps [K,B,1,M,T]. `bounds` = the plan's batch halves (`pl.bounds`; default one half). With
    want_radius every normal tensor `k` comes with `k + "_r"`, the Box-Muller radius of each element (see normal_bound). The values do not
    depend on the frame bucket the model pads T to."""
    import torch
    bounds = [0, B] if bounds is None else list(bounds)
    out = {}
    z0, r0 = fill_normal_rows(2 * B, T, make_key(KEY_F0_Z0, seed), want_radius=True)
    zs, us, rs = [], [], []
    for s in range(steps_f0):
        z, u, r = f0_step_draws(2 * B, T, s, make_key(KEY_F0_STEPS, seed), want_radius=True)
        zs.append(z), us.append(u), rs.append(r)
    zs, us, rs = np.stack(zs), np.stack(us), np.stack(rs)     # [S, 2B, T], [S, 2B, 2, T]
    for g, net in enumerate(("f0_a", "f0_b")):                # net 0 = items [0, B), net 1 = items [B, 2B) of the grouped pair
        sl = slice(g * B, (g + 1) * B)
        d = dict(u_init=np.zeros((B, 1, T)), z0=z0[sl, None], z_steps=zs[:, sl, None], u_steps=us[:, sl])
        if want_radius:
            d.update(z0_r=r0[sl, None], z_steps_r=rs[:, sl, None])
        out[net] = d
    zq, rq = mel_qsample_noise(B, T, M, make_key(KEY_MEL_Q, seed), want_radius=True)     # [B, T, M]
    zm = np.empty((steps_mel, B, T, M))
    rm = np.empty((steps_mel, B, T, M))
    for i in range(len(bounds) - 1):
        b0, nb = bounds[i], bounds[i + 1] - bounds[i]
        if nb <= 0:
            continue
        for s in range(steps_mel):                            # the item index restarts at 0 in every half; the half is in the key
            zm[s, b0:b0 + nb], rm[s, b0:b0 + nb] = mel_step_noise(nb, T, M, s, make_key(key_mel_steps(b0), seed), want_radius=True)
    mel = dict(z_q=zq.transpose(0, 2, 1)[:, None], z_steps=zm.transpose(0, 1, 3, 2)[:, :, None])
    if want_radius:
        mel.update(z_q_r=rq.transpose(0, 2, 1)[:, None], z_steps_r=rm.transpose(0, 1, 3, 2)[:, :, None])
    out["mel"] = mel
    return {k: {kk: torch.from_numpy(np.ascontiguousarray(vv)) for kk, vv in v.items()} for k, v in out.items()}


def vocoder_noise(seed, B, L, NH=9):
    """What `HifiGanGeneratorHIP.forward(..., seed=seed)` draws (the key is `seed` itself): the dict `synth.draw_vocoder_noise` returns."""
    import torch
    return dict(rand_ini=torch.from_numpy(rand_ini(B, make_key(0, seed), NH)), sine_noise=torch.from_numpy(sine_noise(B, L, make_key(0, seed), NH)))


class ReplayTape:
    """`synth.NoiseTape`-compatible source that serves a `model_noise` dict in the reference's order (oracle/restatement.py:
    per f0 sampler rand[B,1,T], randn[B,1,T], then per step (descending) randn[B,1,T], rand[B,2,T]; mel: randn[B,1,M,T], per step randn)."""

    def __init__(self, noise, dtype=None):
        import torch
        dtype = dtype or torch.float32
        q = []
        for net in ("f0_a", "f0_b"):
            d = noise[net]
            q += [("rand", d["u_init"]), ("randn", d["z0"])]
            for i in reversed(range(d["z_steps"].shape[0])):
                q += [("randn", d["z_steps"][i]), ("rand", d["u_steps"][i])]
        m = noise["mel"]
        q.append(("randn", m["z_q"]))
        for i in reversed(range(m["z_steps"].shape[0])):
            q.append(("randn", m["z_steps"][i]))
        self.queue = [(k, t.to(dtype)) for k, t in q]
        self.pos = 0

    def _next(self, kind, shape):
        k, t = self.queue[self.pos]
        assert k == kind and tuple(t.shape) == tuple(shape), f"draw {self.pos}: the oracle asks {kind}{tuple(shape)}, the tape holds {k}{tuple(t.shape)}"
        self.pos += 1
        return t.clone()

    def randn(self, *shape):
        return self._next("randn", shape)

    def rand(self, *shape):
        return self._next("rand", shape)


# ------------------------------------------------------------------------------------------------
# which blocks does a run touch?  (computed from the layouts, not enumerated)
# ------------------------------------------------------------------------------------------------
def _box(site, key, fn, ranges, words):
    """The blocks of one launch sequence as a box: every index of `ranges` = {name: (lo, hi)} (inclusive) runs over its whole range, and every
    counter word of the layouts above is monotone in every index, so the word's extremes are at the corners. `raw_max`: the largest value of
    every word BEFORE the kernel's cast to uint32_t (the 64-bit counters are split by the kernel, not cast)."""
    names = list(ranges)
    lo, hi = [None] * 4, [None] * 4
    for corner in range(1 << len(names)):
        c = fn(**{n: ranges[n][(corner >> j) & 1] for j, n in enumerate(names)})
        for w in range(4):
            lo[w] = c[w] if lo[w] is None else min(lo[w], c[w])
            hi[w] = c[w] if hi[w] is None else max(hi[w], c[w])
    return dict(site=site, key=key, lo=tuple(int(v) for v in lo), hi=tuple(int(v) for v in hi), words=words)


def _box64(site, key, ctr_lo, ctr_hi, c2, c3, words):
    """a 64-bit counter range [ctr_lo, ctr_hi] split into (c0, c1): exact when it stays inside one high word, else c0 is the full range"""
    same = (ctr_lo >> 32) == (ctr_hi >> 32)
    return dict(site=site, key=key, lo=((ctr_lo & M32) if same else 0, ctr_lo >> 32, c2, c3), hi=((ctr_hi & M32) if same else M32, ctr_hi >> 32, c2, c3),
                words=words)


def run_blocks(seed, B, T, steps_f0, steps_mel, bounds=None, M=80, L=None, NH=9, vocoder_seed=None):
    """Every (key, counter box) one forward of the acoustic model (default sampler) and one of the vocoder touch, as a list of dicts
    {site, key, lo[4], hi[4], words}. Two draws share a block only if their keys are equal and their boxes meet in all four words."""
    bounds = [0, B] if bounds is None else list(bounds)
    T4 = (T + 3) // 4
    out = [_box("f0_z0", make_key(KEY_F0_Z0, seed), ctr_fill_normal_rows, dict(t4=(0, T4 - 1), b=(0, 2 * B - 1)), "z0..z3"),
           _box("f0_step", make_key(KEY_F0_STEPS, seed), ctr_f0_step, dict(t=(0, T - 1), b=(0, 2 * B - 1), step=(0, steps_f0 - 1)), "z0,u0,u1"),
           _box("mel_qsample", make_key(KEY_MEL_Q, seed), lambda t, c, b: ctr_mel_qsample(t, c, b, M), dict(t=(0, T - 1), c=(0, M - 1), b=(0, B - 1)), "z0")]
    for i in range(len(bounds) - 1):
        nb = bounds[i + 1] - bounds[i]
        if nb > 0:   # sigma = 0 at step 0: no draw there, but counting it costs nothing
            out.append(_box(f"mel_step[half {i}]", make_key(key_mel_steps(bounds[i]), seed), lambda t4, n, b, step: ctr_mel_step(t4, n, b, step, M),
                            dict(t4=(0, T4 - 1), n=(0, M - 1), b=(0, nb - 1), step=(0, steps_mel - 1)), "z0..z3"))
    if L is not None:
        vkey = make_key(0, seed if vocoder_seed is None else vocoder_seed)
        out.append(_box("rand_ini", vkey, lambda b, h: ctr_rand_ini(b, h, NH), dict(b=(0, B - 1), h=(1, NH - 1)), "u"))
        out.append(_box64("sine_noise", vkey, 0, B * L * NH - 1, TAG_SINE, TAG_NSF2, "z0"))
    return out


def boxes_meet(a, b):
    return all(a["lo"][w] <= b["hi"][w] and b["lo"][w] <= a["hi"][w] for w in range(4))
