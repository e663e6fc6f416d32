"""numpy emulation of the fp16 two-term split (csrc/m4d_wino_f16.hip) against the bf16 three-term split (csrc/m4d_wino6.hip)
and a float32 chain: dot products of leaky-relu'd Winograd-like operands (three magnitude classes) with N(0, 0.04^2) weights,
error against float64 in units of the dot product's rms.  An EMULATION, not the matrix core: every group of 16 exact products
is summed exactly and rounded once into the float32 accumulator (the model assumed for v_mfma_f32_32x32x16_{f16,bf16}).

    python tools/probes/f16x2_split_emulation.py [--rows 256] [--cols 64]
"""
import argparse

import numpy as np


def bf16_rn(x):
    u = x.astype(np.float32).view(np.uint32).astype(np.uint64)
    return ((((u + 0x7FFF + ((u >> 16) & 1)) >> 16) & 0xFFFF) << 16).astype(np.uint32).view(np.float32)


def split_bf16x3(x):
    p1 = bf16_rn(x); r = (x - p1).astype(np.float32)
    p2 = bf16_rn(r); p3 = (r - p2).astype(np.float32)
    return [p1, p2, p3]


def split_f16x2(x, scale_axis):
    """2^s per row (scale_axis=1: per row of A) or per column (scale_axis=0: per column of B), |2^s x| < 2^15."""
    amax = np.abs(x).max(axis=scale_axis, keepdims=True).astype(np.float64)
    s = np.where(amax > 0, 15 - np.frexp(amax)[1], 0)
    xs = x.astype(np.float64) * np.ldexp(1.0, s)
    hi = xs.astype(np.float16).astype(np.float64)
    lo = (xs - hi).astype(np.float16).astype(np.float64)
    return hi, lo, s


def mfma_chain(terms, K):
    """sum over (a, b) term pairs of A @ B, 16 k at a time, each group rounded once into a float32 accumulator."""
    acc = np.zeros((terms[0][0].shape[0], terms[0][1].shape[1]), np.float32)
    for k0 in range(0, K, 16):
        for a, b in terms:
            acc = (acc.astype(np.float64) + a[:, k0:k0 + 16].astype(np.float64) @ b[k0:k0 + 16].astype(np.float64)).astype(np.float32)
    return acc.astype(np.float64)


def fp32_chain(A, B):
    acc = np.zeros((A.shape[0], B.shape[1]), np.float32)
    for k in range(A.shape[1]):
        acc = (acc + (A[:, k:k + 1] * B[k:k + 1]).astype(np.float32)).astype(np.float32)
    return acc.astype(np.float64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=256)
    ap.add_argument("--cols", type=int, default=64)
    args = ap.parse_args()
    rng = np.random.default_rng(0)
    for K in (16, 128, 1152):
        mags = np.repeat(np.array([1e-3, 1.0, 1e3], np.float32), -(-args.rows // 3))[:args.rows, None]
        d = rng.standard_normal((args.rows, K)).astype(np.float32)
        A = (np.where(d > 0, d, 0.1 * d) * mags * 2.0).astype(np.float32)          # leaky-relu'd, Winograd-transform-sized
        B = (0.04 * rng.standard_normal((K, args.cols))).astype(np.float32)
        truth = A.astype(np.float64) @ B.astype(np.float64)
        rms = np.sqrt((truth ** 2).mean(axis=1, keepdims=True))
        err = lambda c: np.abs(c - truth) / rms
        e32 = err(fp32_chain(A, B))
        a3, b3 = split_bf16x3(A), split_bf16x3(B)
        e_bf = err(mfma_chain([(a3[2], b3[0]), (a3[0], b3[2]), (a3[1], b3[1]), (a3[1], b3[0]), (a3[0], b3[1]), (a3[0], b3[0])], K))
        ah, al, sa = split_f16x2(A, 1)
        bh, bl, sb = split_f16x2(B, 0)
        c = mfma_chain([(al, bh), (ah, bl), (ah, bh)], K) * np.ldexp(1.0, -sa) * np.ldexp(1.0, -sb)
        e_f16 = err(c)
        print(f"K {K:5d}: mean error / rms -- fp32 chain {e32.mean():.2e}, bf16x3 (6 products) {e_bf.mean():.2e}, "
              f"f16x2 (3 products, scale per row) {e_f16.mean():.2e} (max {e_f16.max():.2e})")


if __name__ == "__main__":
    main()
