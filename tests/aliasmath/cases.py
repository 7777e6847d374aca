"""The input set of the alias-table build tests (tests/test_alias_device_cpu.py, tests/test_alias_device_gpu.py): five kinds of powers at each size."""
import numpy as np

SIZES = (1, 2, 7, 8, 15, 16, 17, 33, 1000, 4097)
# the block, wave and sum-chunk boundaries of zr_tu_alias.hip, and more lights than the atrium's 100 000 (not a multiple of anything)
SIZES_GPU_EXTRA = (63, 64, 65, 255, 256, 257, 100003)
KINDS = ("equal", "one_heavy", "one_zero", "span", "log_uniform")
# beyond the input set: sizes where one light's fixed-point weight passes 2^48 -- almost all the power in one light, and one light with a fifth of it
LARGE_CASES = (("one_heavy", 100003), ("one_fifth", 100000), ("one_fifth", 40000), ("log_uniform", 100003))


def powers(kind, n):
    if kind == "one_fifth":
        p = np.ones(n, np.float32)
        p[n // 7] = n / 4.0                                 # 0.25 n of 1.25 n
        return p
    rng = np.random.default_rng(1000 * KINDS.index(kind) + n)
    if kind == "equal":
        p = np.full(n, 0.3, np.float32)                     # 0.3f * n is not exact: probs are 1 - 2^-24 or so, not 1
    elif kind == "one_heavy":
        p = np.full(n, 1e-6, np.float32)
        p[n // 3] = 5000.0
    elif kind == "one_zero":
        p = rng.uniform(0.5, 2.0, n).astype(np.float32)
        p[n // 2] = 0.0
        if n == 1:
            p[0] = 1.0                                      # (a lone light must carry the positive sum)
    elif kind == "span":
        p = np.exp2(np.linspace(-40.0, 20.0, n)).astype(np.float32)
        p = p[rng.permutation(n)]
    else:
        p = np.exp(rng.uniform(np.log(1e-4), np.log(1e4), n)).astype(np.float32)
    return p


def all_cases(sizes=SIZES):
    return [(k, n) for n in sizes for k in KINDS]


def represented(table):
    """float64: the probability the table gives each light, q_i = (p_curr_i + sum over j != i with alias_j == i of (1 - p_curr_j)) / n"""
    n = len(table)
    p = table["p_curr"].astype(np.float64)
    a = table["alias"].astype(np.int64)
    q = p.copy()
    other = a != np.arange(n)
    np.add.at(q, a[other], 1.0 - p[other])
    return q / n


def validity_excess(table, power):
    """max over i of |q_i - p_i| / (2^-21 p_i + 2^-30 / n), p_i = power_i / sum of the powers in float64: <= 1 is a valid table"""
    n = len(table)
    pw = power.astype(np.float64)
    p = pw / pw.sum()
    bound = 2.0 ** -21 * p + 2.0 ** -30 / n
    return float((np.abs(represented(table) - p) / bound).max())
