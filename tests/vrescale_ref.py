"""float64 numpy restatement of the stochastic velocity-rescaling thermostat (admp_amd/csrc/md_vrescale_math.h, with the
generator of md_math.h): Philox-4x32-10, the normals, the noise (R1, S, tries) of one (seed, step) and one application of the
rule.  Shared by tests/test_md_vrescale_cpu.py (which holds the header to it) and tests/test_gpu_md_vrescale.py (which holds the
kernels to it).  Not a test module."""
import math

import numpy as np

ACC = 1e-4                 # 1 kJ/mol/A/amu = 1e-4 A/fs^2
KB = 0.0083144626          # kJ/mol/K
STREAM = 3                 # kStreamVRescale
K_BEFORE, K_AFTER, ALPHA, HEAT, APPLICATIONS, TRIES, RESERVED, FLAGS = range(8)
FAILED = 1.0
MAX_TRIES = 64
M0, M1, W0, W1, LOW = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85, 0xffffffff


def fresh_state():
    return np.array([0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0])


def philox(counter, key):
    """four 32-bit counter words and two key words (python ints) -> four 32-bit words"""
    c0, c1, c2, c3 = counter
    k0, k1 = key
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & LOW, (p0 >> 32) ^ c3 ^ k1, p0 & LOW
        k0, k1 = (k0 + W0) & LOW, (k1 + W1) & LOW
    return c0, c1, c2, c3


def words(seed, step, index, stream=STREAM):
    return philox((index, step & LOW, step >> 32, stream), (seed & LOW, seed >> 32))


def normals(w):
    """the three normals of one counter's words"""
    u = [(x + 0.5) * 2.0 ** -32 for x in w]
    r0, r1 = math.sqrt(-2.0 * math.log(u[0])), math.sqrt(-2.0 * math.log(u[2]))
    return r0 * math.cos(2.0 * math.pi * u[1]), r0 * math.sin(2.0 * math.pi * u[1]), r1 * math.cos(2.0 * math.pi * u[3])


def noise(seed, step, n_dof):
    """(R1, S, tries); tries = 0 where no gamma deviate is needed, -1 when MAX_TRIES were rejected"""
    xi = normals(words(seed, step, 0))
    rest = n_dof - 1
    a = rest // 2
    S = xi[1] * xi[1] if rest % 2 else 0.0
    if a < 1:
        return xi[0], S, 0
    d = a - 1.0 / 3.0
    q = 1.0 / math.sqrt(9.0 * d)
    for t in range(MAX_TRIES):
        w = words(seed, step, 1 + t)
        x = normals(w)[0]
        u = (w[2] + 0.5) * 2.0 ** -32
        v = (1.0 + q * x) ** 3
        if v > 0.0 and math.log(u) < 0.5 * x * x + d - d * v + d * math.log(v):
            return xi[0], S + 2.0 * d * v, t + 1
    return xi[0], S, -1


def noise_many(seed, steps, n_dof):
    """the same for an array of steps at once (numpy throughout): arrays (R1, S, tries)"""
    steps = np.asarray(steps, dtype=np.uint64)
    n = len(steps)

    def phil(index):
        full = lambda x: np.full(n, x, dtype=np.uint64)      # noqa: E731
        c = [full(index), steps & np.uint64(LOW), steps >> np.uint64(32), full(STREAM)]
        k0, k1 = seed & LOW, seed >> 32
        for _ in range(10):
            p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]
            c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & np.uint64(LOW), (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1),
                 p0 & np.uint64(LOW)]
            k0, k1 = (k0 + W0) & LOW, (k1 + W1) & LOW
        return (np.stack(c, axis=1).astype(np.float64) + 0.5) * 2.0 ** -32

    u = phil(0)
    r0 = np.sqrt(-2.0 * np.log(u[:, 0]))
    R1, x1 = r0 * np.cos(2.0 * np.pi * u[:, 1]), r0 * np.sin(2.0 * np.pi * u[:, 1])
    rest = n_dof - 1
    a = rest // 2
    S = x1 * x1 if rest % 2 else np.zeros(n)
    tries = np.zeros(n, dtype=np.int64)
    if a < 1:
        return R1, S, tries
    d = a - 1.0 / 3.0
    q = 1.0 / math.sqrt(9.0 * d)
    open_ = np.ones(n, dtype=bool)
    for t in range(MAX_TRIES):
        u = phil(1 + t)
        x = np.sqrt(-2.0 * np.log(u[:, 0])) * np.cos(2.0 * np.pi * u[:, 1])
        v = (1.0 + q * x) ** 3
        with np.errstate(invalid='ignore', divide='ignore'):
            ok = open_ & (v > 0.0) & (np.log(u[:, 2]) < 0.5 * x * x + d - d * v + d * np.log(v))
        S = np.where(ok, S + 2.0 * d * v, S)
        tries[ok] = t + 1
        open_ &= ~ok
        if not open_.any():
            break
    tries[open_] = -1
    return R1, S, tries


def rule(state, K, n_dof, kT_acc, c, seed, step, real=np.float64):
    """(state', alpha, scales): one application for velocities of type `real`"""
    state = np.asarray(state, dtype=np.float64)
    out = state.copy()
    if state[FLAGS] == FAILED:
        return out, 1.0, False
    if not math.isfinite(K):
        out[FLAGS] = FAILED
        return out, 1.0, False
    alpha, tries = 1.0, 0
    if K > 0.0 and c < 1.0:
        R1, S, tries = noise(seed, step, n_dof)
        g = (1.0 - c) * (0.5 * kT_acc)
        r = math.sqrt(c * K) + math.sqrt(g) * R1
        alpha = math.sqrt((r * r + g * S) / K)
        if tries < 0 or not math.isfinite(alpha):
            out[FLAGS] = FAILED
            return out, 1.0, False
    at = float(real(alpha))
    K_after = at * at * K
    out[:7] = K, K_after, alpha, state[HEAT] + (K_after - K), state[APPLICATIONS] + 1.0, float(tries), 0.0
    return out, alpha, True


def kinetic(v, inv_mass):
    """sum v^2 / inv_mass / 2 of (n,3) velocities in float64"""
    v = np.asarray(v, dtype=np.float64)
    return float(0.5 * ((v * v).sum(1) / np.asarray(inv_mass, dtype=np.float64)).sum())
