"""numpy emulation of criteria_sums_kernel's summation scheme (ssl_amd/csrc/ssg_grow.hip) at the smallest size at which
every lane flushes its fp32 run: how far a CORRECT kernel is from the fp64 sums, to show that the 2e-6 bound of
tests/test_gpu_ref_api.py leaves room at 69,206,019 elements.  No GPU; about a minute and 3 GB.

The aligned path: 2,048 x 256 lanes, lane L takes the float4 L + k * 524,288 on trip k and adds its four terms in order
into two fp32 sums; after 32 trips (128 terms) the fp32 sums go to fp64 and restart.  The three tail elements go to the
fp32 sums of lanes 0..2.  Everything beyond a lane is fp64 (its order moves the result by ~1e-16 and is not restated).
The terms are criteria_elem's: |a - b|, and fl32(t' * fl32(ln 2 * log2(fl32(t' / s')))) with both clamped at 1e-10.

    python tools/criteria_flush_emulation.py            # prints the two relative errors
"""
import sys

import numpy as np

GRID, NT, RUN = 2048, 256, 32


def inputs(n, seed=23):
    """The recipe of the criteria tests: rand ** 6, zero blocks, exact ties, one 3e-11 element."""
    rng = np.random.default_rng(seed)
    a = rng.random(n, dtype=np.float32) ** np.float32(6)
    b = rng.random(n, dtype=np.float32) ** np.float32(6)
    a[:50] = 0.0
    b[25:75] = 0.0
    a[100:120] = b[100:120]
    a[200] = 3e-11
    return a, b


def terms(a, b):
    cl = np.float32(1e-10)
    ac, bc = np.maximum(a, cl), np.maximum(b, cl)
    ratio = (bc.astype(np.float64) / ac.astype(np.float64)).astype(np.float32)      # correctly rounded quotient
    kl = bc * (np.float32(0.69314718056) * np.log2(ratio.astype(np.float64)).astype(np.float32))
    return np.abs(a - b), kl, ac, bc


def kernel_scheme(t, n):
    """Sum of the fp32 terms t[:n] as the aligned path forms it."""
    lanes = GRID * NT
    n4 = n // 4
    trips = -(-n4 // lanes)
    full = np.zeros(trips * lanes * 4, np.float32)
    full[:4 * n4] = t[:4 * n4]
    full = full.reshape(trips, lanes, 4)
    acc64 = np.zeros(lanes, np.float64)
    acc32 = np.zeros(lanes, np.float32)
    run = 0
    for k in range(trips):          # (a lane without a float4 on the last trip adds zeros and flushes nothing new)
        for c in range(4):
            acc32 = acc32 + full[k, :, c]
        run += 1
        if run == RUN:
            acc64 += acc32.astype(np.float64)
            acc32 = np.zeros(lanes, np.float32)
            run = 0
    tail = t[4 * n4:n]
    acc32[:tail.size] = acc32[:tail.size] + tail
    acc64 += acc32.astype(np.float64)
    return float(acc64.sum())


def main(n=33 * 4 * GRID * NT + 3):
    a, b = inputs(n)
    l1, kl, ac, bc = terms(a, b)
    l1_64 = float(np.abs(a.astype(np.float64) - b.astype(np.float64)).sum())
    bc64, ac64 = bc.astype(np.float64), ac.astype(np.float64)
    kl_64 = float((bc64 * (np.log(bc64) - np.log(ac64))).sum())
    e1 = abs(kernel_scheme(l1, n) - l1_64) / abs(l1_64)
    e2 = abs(kernel_scheme(kl, n) - kl_64) / abs(kl_64)
    print(f"n {n}: fp32 runs of {4 * RUN}, fp64 beyond, against the fp64 sums: L1 {e1:.2e} relative, KL {e2:.2e} relative")


if __name__ == "__main__":
    main(*(int(v) for v in sys.argv[1:2]))
