"""Crafted initial accumulators for the rotations and crafted inputs for the trace (test infrastructure).

The stage entries omr_blind_rotate_level{1,2}_from take the initial accumulator from the caller, and
omr_trace takes any RLWE. Two facts make every decomposition input reachable:

- with the rotation amount a = N, (X^a - 1) ACC = -2 ACC, and q is odd, so the decomposition input T
  is reached with ACC = -T 2^-1 mod q (acc_for_target);
- a step with a_i = 0 is skipped, so an LWE with one nonzero a_i runs exactly one CMUX step, on the key
  rows of step i.

Every function is deterministic, pure numpy plus the oracle, and returns (lwe, acc0) for one message
(the trace functions: one RLWE). cases(level, dk) / trace_cases(dk) give the whole named set, about a
dozen messages each (level 2: 19, with the cases for the two-CU latency kernels). tests/test_acc_cases_host.py proves on the CPU that the set holds what it claims.
"""
import numpy as np

import oracle_lib as O

Q1 = 134215681
Q2 = 1125899906826241


class Level:
    def __init__(self, level, q, N, logB, d, drop, n_lwe, which):
        self.level, self.q, self.N, self.logB, self.d, self.drop, self.n_lwe, self.which = \
            level, q, N, logB, d, drop, n_lwe, which
        self.B = 1 << logB
        self.h = (q - 1) // 2
        self.n = N // 2  # complex points of the folded transform

    @property
    def last_step(self):
        return self.n_lwe - 1


L1 = Level(1, Q1, 1024, 5, 4, 7, 512, 1)
L2 = Level(2, Q2, 2048, 7, 6, 8, 670, 2)
LT = Level(3, Q2, 2048, 2, 25, 0, 0, 3)  # the trace basis (no LWE)
LEVELS = {1: L1, 2: L2}


# ---- residues --------------------------------------------------------------------------------------
def centred(v, q):
    v = int(v) % q
    return v - q if v > (q - 1) // 2 else v


def canon_array(vals, q):
    """Python integers (any representative) -> canonical u64 array."""
    return np.array([int(v) % q for v in vals], dtype=np.uint64)


def acc_for_target(T, q):
    """ACC with -2 ACC = T (mod q), coefficient-wise: what a step with a = N decomposes."""
    inv2 = (q + 1) // 2
    return canon_array([(-int(t) * inv2) % q for t in T], q)


def decompose(L, x):
    """Digits of the canonical residue x under the oracle (oref_decompose)."""
    dg = np.zeros(32, dtype=np.int64)
    n = O.lib().oref_decompose(L.which, int(x) % L.q, dg)
    return [int(v) for v in dg[:n]]


def from_digits(L, digits):
    """The centred residue (sum_k d_k B^k) 2^drop whose decomposition is `digits` (when it is balanced and
    within +-h; callers check with decompose)."""
    return sum(int(dk) << (L.logB * k) for k, dk in enumerate(digits)) << L.drop


def carry_chain(L, T):
    """Longest run of consecutive carries in the decomposition of the centred residue T in which every carry
    after the first happens only because of the carry coming in (the digit below it was B/2 - 1 before
    the carry arrived)."""
    y = (int(T) + ((1 << (L.drop - 1)) if L.drop else 0)) >> L.drop
    best = run = cin = 0
    for _ in range(L.d - 1):
        carried = (y % L.B) >= L.B // 2
        induced = carried and cin == 1 and ((y - 1) % L.B) < L.B // 2
        run = run + 1 if induced else (1 if carried else 0)
        best = max(best, run)
        cin = 1 if carried else 0
        y = (y + L.B // 2) >> L.logB
    return best


def chain_value(L, length, negative=False):
    """A y (before the drop) whose decomposition carries `length` times in a row from digit 0: digit 0 is
    B/2, the next length - 1 are B/2 - 1. negative: the same low digits under a top digit of -1, a negative
    residue (the carries depend on the low digits alone)."""
    y = L.B // 2 + sum((L.B // 2 - 1) << (L.logB * k) for k in range(1, length))
    return y - (1 << (L.logB * (L.d - 1))) if negative else y


def top_range(L):
    """(min, max) of the top digit over all residues."""
    return decompose(L, -L.h)[-1], decompose(L, L.h)[-1]


# ---- the LWE ---------------------------------------------------------------------------------------
def lwe_for(L, steps):
    """An LWE whose only nonzero mask entries are steps[i] = a_i (the body is unused by the _from entries)."""
    if L.level == 1:
        a = np.zeros(L.n_lwe, dtype=np.uint16)
    else:
        a = np.zeros(L.n_lwe + 1, dtype=np.uint32)
    for i, v in steps.items():
        assert 0 < v < 2 * L.N
        a[i] = v
    return a


def first_step(L, lwe):
    i = int(np.flatnonzero(np.asarray(lwe)[:L.n_lwe])[0])
    return i, int(lwe[i])


def step_input(L, acc_poly, a):
    """(X^a - 1) * ACC mod q for one polynomial: the first step's decomposition input, canonical."""
    rot = np.zeros(L.N, dtype=np.uint64)
    O.lib().oref_negacyclic_mul_monomial(L.level, np.ascontiguousarray(acc_poly, dtype=np.uint64), a, rot)
    return canon_array([int(r) - int(c) for r, c in zip(rot, acc_poly)], L.q)


# ---- boundary residues -----------------------------------------------------------------------------
def boundary_targets(L):
    """Centred residues T a decomposition must get right: the residue extremes, the drop-rounding ties in
    both signs, every digit position at its minimum and maximum (the top digit at +B/2 and at its
    minimum), and carry chains of every length up to d - 1 in both signs."""
    h, B, half = L.h, L.B, (1 << (L.drop - 1)) if L.drop else 0
    t = [0, 1, -1, h, -h, h - 1, -(h - 1)]
    if L.drop:
        for k in (0, 1, 12345):
            for r in (half - 1, half, half + 1):
                t += [(k << L.drop) + r, -((k << L.drop) + r)]
    for k in range(L.d - 1):
        for v in (-(B // 2), B // 2 - 1):
            dg = [0] * L.d
            dg[k] = v
            t.append(from_digits(L, dg))
            dg = [1] * L.d  # the same digit among nonzero neighbours
            dg[k] = v
            t.append(from_digits(L, dg))
    # (the top digit's extremes are those of +-h, above: the maximum is +B/2 at both levels)
    for length in range(1, L.d):
        t += [chain_value(L, length) << L.drop, chain_value(L, length, True) << L.drop]
    assert all(abs(v) <= h for v in t)
    return t


def _fill(L, seed):
    return [int(v) for v in np.random.default_rng(seed).integers(0, L.q, L.N, dtype=np.uint64)]


def _place(L, base, targets, stride, offset):
    out = list(base)
    for k, v in enumerate(targets):
        out[(offset + k * stride) % L.N] = v
    return out


def boundary_case(L, variant=0, steps=None):
    """One step with a = N on an accumulator whose decomposition inputs hold boundary_targets at spread
    coefficients among random residues. variant 0: targets in both polynomials; 1: an all-zero mask
    polynomial with the targets in the body; 2: the reverse. steps: the LWE's nonzero entries
    (default: step 0 with a = N)."""
    tg = boundary_targets(L)
    stride = L.N // len(tg) if len(tg) <= L.N else 1
    assert len(tg) * stride <= L.N
    Ta = _place(L, _fill(L, 10 + L.level), tg, stride, 0)
    Tb = _place(L, _fill(L, 20 + L.level), tg[::-1], stride, 3)
    if variant == 1:
        Ta = [0] * L.N
    elif variant == 2:
        Tb = [0] * L.N
    acc0 = np.stack([acc_for_target(Ta, L.q), acc_for_target(Tb, L.q)])
    return lwe_for(L, steps or {0: L.N}), acc0


PRE_REDUCTION_A = lambda L: (1, L.N - 1, L.N + 1, 2 * L.N - 1)  # noqa: E731


def pre_reduction_case(L, a):
    """rot - acc = +-(q - 1) before reduction: pairs ACC_j = +-h against the rotated entry -+h (two
    two-coefficient supports per polynomial, one per sign), for a general rotation amount a. Returns
    (lwe, acc0); pre_reduction_sites(L, a) names the coefficients."""
    acc = [[0] * L.N, [0] * L.N]
    for p in range(2):
        for j, src, sign, s in pre_reduction_sites(L, a):
            acc[p][j] = s * L.h            # acc_j = s h
            acc[p][src] = -s * sign * L.h  # rot_j = sign * acc_src = -s h
    return lwe_for(L, {0: a}), np.stack([canon_array(acc[0], L.q), canon_array(acc[1], L.q)])


def pre_reduction_sites(L, a):
    """(j, src, sign, s): coefficient j reads rot_j = sign * ACC_src; s = the sign of ACC_j."""
    sites = []
    for j, s in ((5, 1), (L.N // 2 + 7, -1)):
        u = (j - a) % (2 * L.N)
        sites.append((j, u % L.N, -1 if u >= L.N else 1, s))
    used = [x for st in sites for x in st[:2]]
    assert len(set(used)) == len(used)
    return sites


# ---- spectrally aligned worst case -----------------------------------------------------------------
def _twist(n):
    return np.exp(1j * np.pi * np.arange(n) / (2 * n))


def folded_spectrum(p, n):
    """The folded, twisted transform of a coefficient-domain polynomial (2n real values), unnormalised:
    S[m] = sum_k (p_k + i p_{k+n}) e^{i pi k / 2n} e^{-2 pi i k m / n} (fft_bound.py's, times n)."""
    p = np.asarray(p, dtype=np.float64)
    return np.fft.fft((p[..., :n] + 1j * p[..., n:]) * _twist(n), axis=-1)


def _centred_f(v, q):
    v = np.asarray(v).astype(np.int64)
    return np.where(v > (q - 1) // 2, v - q, v).astype(np.float64)


def key_step_rows(L, dk, i):
    """The centred key rows of step i as fft_bound.py splits them: [rows][outputs (* limbs)][2n]."""
    if L.level == 1:
        return _centred_f(dk.bsk1.reshape(512, 8, 2, 1024)[i], Q1)
    key = dk.bsk2.reshape(670, 12, 2, 2048) if L.level == 2 else dk.trace_key.reshape(11, 25, 2, 2048)
    r = _centred_f(key[i], Q2)
    hi = np.rint(r / 2.0 ** 25)
    return np.stack([r - hi * 2.0 ** 25, hi], axis=-2).reshape(r.shape[0], 4, 2048)


_PEAKS = {}


def spectral_peak(L, dk):
    """(step i*, row, output(-limb), point m*, kappa): where the key's spectrum is largest, the kappa of
    fft_bound.py (for the trace: over the first automorphism step, the one that sees the input)."""
    key = (L.level, id(dk))
    if key not in _PEAKS:
        best = (0.0,)
        steps = {1: 512, 2: 670, 3: 1}[L.level]
        for i in range(steps):
            mag = np.abs(folded_spectrum(key_step_rows(L, dk, i), L.n)) / L.n
            k = float(mag.max())
            if k > best[0]:
                r, o, m = np.unravel_index(int(mag.argmax()), mag.shape)
                best = (k, i, int(r), int(o), int(m))
        _PEAKS[key] = (best[1], best[2], best[3], best[4], best[0])
    return _PEAKS[key]


def aligned_signs(n, m):
    """crafted_keys.aligned_row's signs at point m instead of 0: s (2n values +-1) with
    Re((s_k + i s_{k+n}) e^{i phi_k}) = |cos phi_k| + |sin phi_k|, phi_k = pi k / 2n - 2 pi k m / n, so that
    the folded spectrum of s at m is real and about (4 / pi) n = 1.27 n."""
    k = np.arange(n)
    phi = np.pi * k / (2 * n) - 2 * np.pi * k * m / n
    re = np.where(np.cos(phi) >= 0, 1, -1)
    im = np.where(np.sin(phi) >= 0, -1, 1)
    return np.concatenate([re, im]).astype(np.int64)


def extreme_digits(L):
    """(digits for sign +, digits for sign -): every digit at its largest magnitude of that sign for which
    the residue stays within +-h and oref_decompose returns exactly these digits. Below the top: B/2 - 1
    and -B/2. All digits at the extreme overflow h (level 2: six digits of -64), so the top digit is the
    largest that still fits."""
    out = []
    for low, step in ((L.B // 2 - 1, -1), (-(L.B // 2), 1)):
        tmin, tmax = top_range(L)
        top = tmax if step == -1 else tmin
        while True:
            dg = [low] * (L.d - 1) + [top]
            T = from_digits(L, dg)
            if abs(T) <= L.h and decompose(L, T) == dg:
                break
            top += step
        out.append(dg)
    return out[0], out[1]


def targets_from_signs(L, signs):
    pos, neg = extreme_digits(L)
    tp, tn = from_digits(L, pos), from_digits(L, neg)
    return [tp if s > 0 else tn for s in signs]


def spectral_case(L, dk):
    """One step i* (a = N) whose digit polynomials -- all 2d of them, both polynomials alike -- have the
    largest magnitude at every coefficient, with signs aligned to the spectral point m* where the key's
    spectrum peaks."""
    i, _, _, m, _ = spectral_peak(L, dk)
    T = targets_from_signs(L, aligned_signs(L.n, m))
    acc = acc_for_target(T, L.q)
    return lwe_for(L, {i: L.N}), np.stack([acc, acc])


COEF_ALIGNED = lambda L: (0, L.N // 2 - 1, L.N - 1)  # noqa: E731


def coefficient_case(L, dk, c):
    """test_gpu_fft1_product_exact's alignment against the real key: digits of the largest magnitude whose
    signs follow the peak row's, so that every term of output coefficient c of digit * row has one sign
    (out_c = sum_j d_j k_{c-j}, negated when wrapped). Level 2: the row's low 25-bit limb."""
    i, r, o, _, _ = spectral_peak(L, dk)
    row = key_step_rows(L, dk, i)[r, o]
    j = np.arange(L.N)
    wrap = np.where(j <= c, 1, -1)
    s = wrap * np.where(row[(c - j) % L.N] >= 0, 1, -1)
    acc = acc_for_target(targets_from_signs(L, s), L.q)
    return lwe_for(L, {i: L.N}), np.stack([acc, acc])


def random_case(L, dk, seed=77):
    """A uniformly random canonical accumulator through the spectral case's single step: the margin the
    aligned cases must exceed."""
    i = spectral_peak(L, dk)[0]
    rng = np.random.default_rng(seed)
    return lwe_for(L, {i: L.N}), rng.integers(0, L.q, (2, L.N), dtype=np.uint64)


# ---- the two-CU schedule (level 2) -----------------------------------------------------------------
# Executed steps of steps_many: boundary targets at step 0, then two consecutive steps, a gap (the key rows
# held for step 3 are not step 7's), and the last two steps (the last one has no next row to load). Six
# hand-offs: each payload slot (the step count's parity) is reused twice, and the key prefetchers' lead of
# two executed steps binds.
STEPS_MANY = lambda L: {0: L.N, 1: 3, 2: L.N + 1, 7: 1, L.last_step - 1: 2 * L.N - 1, L.last_step: L.N}  # noqa: E731


def word_split_digits(L):
    """{"low_zero": (digits +, digits -), "high_zero": (digits +, digits -)}: the lower half of the digits
    (the first digit word of the level-2 FFT kernels: digits 0..2) all zero while the upper half sits at its
    extremes of one sign (the top digit the largest that fits, as in extreme_digits), and the reverse."""
    half = L.d // 2
    pos, neg = extreme_digits(L)
    out = {"high_zero": ([L.B // 2 - 1] * half + [0] * (L.d - half), [-(L.B // 2)] * half + [0] * (L.d - half))}
    low = []
    for ext, step in ((pos, -1), (neg, 1)):
        dg = [0] * half + list(ext[half:])
        while not (abs(from_digits(L, dg)) <= L.h and decompose(L, from_digits(L, dg)) == dg):
            dg[-1] += step
        low.append(dg)
    out["low_zero"] = (low[0], low[1])
    return out


def word_split_case(L, which, poly):
    """One step (a = N) in which every coefficient of polynomial `poly` (0 mask, 1 body) decomposes to
    word_split_digits(L)[which], the sign by a fixed coin per coefficient, and the other polynomial is zero:
    one half of the digit polynomials is all-zero beside a half at its extremes, and the partner polynomial's
    digits are all zero."""
    dp, dn = word_split_digits(L)[which]
    tp, tn = from_digits(L, dp), from_digits(L, dn)
    coin = np.random.default_rng(40 + poly + 2 * (which == "low_zero")).integers(0, 2, L.N)
    acc = acc_for_target([tp if c else tn for c in coin], L.q)
    zero = np.zeros(L.N, dtype=np.uint64)
    return lwe_for(L, {0: L.N}), np.stack([acc, zero] if poly == 0 else [zero, acc])


WORD_SPLIT = [(w, p) for w in ("low_zero", "high_zero") for p in (0, 1)]
word_split_name = lambda which, poly: f"word_split_{which}_{'mask' if poly == 0 else 'body'}"  # noqa: E731


# ---- the sets --------------------------------------------------------------------------------------
def cases(level, dk):
    """name -> (lwe, acc0): the whole set of one level."""
    L = LEVELS[level]
    out = {"boundary": boundary_case(L, 0), "zero_mask": boundary_case(L, 1), "zero_body": boundary_case(L, 2)}
    for a in PRE_REDUCTION_A(L):
        out[f"pre_reduction_a{a}"] = pre_reduction_case(L, a)
    out["spectral"] = spectral_case(L, dk)
    for c in COEF_ALIGNED(L):
        out[f"coef_aligned_{c}"] = coefficient_case(L, dk, c)
    # more than one step: consecutive steps (the next row's prefetch), a gap, the last step
    out["steps_0_1"] = boundary_case(L, 0, {0: L.N, 1: 3})
    out["steps_0_5"] = boundary_case(L, 0, {0: L.N + 1, 5: L.N})
    out["step_last"] = boundary_case(L, 0, {L.last_step: L.N})
    if level == 2:  # the two-CU kernels' schedule and their split of the digits over groups and workgroups
        out["steps_many"] = boundary_case(L, 0, STEPS_MANY(L))
        for which, poly in WORD_SPLIT:
            out[word_split_name(which, poly)] = word_split_case(L, which, poly)
    return out


def aligned_names(level):
    return ["spectral"] + [f"coef_aligned_{c}" for c in COEF_ALIGNED(LEVELS[level])]


def stack(cs, names=None):
    names = list(cs) if names is None else names
    return np.stack([cs[k][0] for k in names]), np.stack([cs[k][1] for k in names])


# ---- the trace -------------------------------------------------------------------------------------
NINV2 = pow(2048, -1, Q2)
SIGMA0 = 2048 + 1  # the first automorphism: g = (N >> 0) + 1


def _sigma0(p):
    out = np.zeros(2048, dtype=np.uint64)
    O.lib().oref_automorphism(np.ascontiguousarray(p, dtype=np.uint64), SIGMA0, out)
    return out


def trace_mask_for(v):
    """The mask a whose first key switch decomposes v: that step sees sigma_g(a N^-1), and sigma_g with
    g = N + 1 is an involution, so a = N sigma_g(v)."""
    s = _sigma0(canon_array(v, Q2))
    return canon_array([int(x) * 2048 for x in s], Q2)


def trace_seen(rlwe):
    """What the first key switch of the trace decomposes: sigma_g(a N^-1), canonical."""
    a = canon_array([int(x) * NINV2 for x in rlwe[0]], Q2)
    return _sigma0(a)


def trace_targets():
    """Residue extremes, base-4 carry chains of every length 1..24 in both signs, every top digit, and v
    whose low 2k bits are all ones-digits (0b0101..) or all twos-digits (0b1010..), in both signs."""
    L = LT
    t = [0, 1, -1, L.h, -L.h, L.h - 1, -(L.h - 1)]
    for length in range(1, L.d):
        t += [chain_value(L, length), chain_value(L, length, True)]
    tmin, tmax = top_range(L)
    for top in range(tmin, tmax + 1):
        v = top << (L.logB * (L.d - 1))
        t.append(max(-L.h, min(L.h, v)))
    for k in range(1, L.d):
        ones = sum(1 << (2 * j) for j in range(k))
        t += [ones, -ones, 2 * ones, -2 * ones]
    assert all(abs(v) <= L.h for v in t)
    return t


def _trace_body(seed):
    return np.random.default_rng(seed).integers(0, Q2, 2048, dtype=np.uint64)


def trace_boundary_case():
    tg = trace_targets()
    stride = 2048 // len(tg)
    v = _place(LT, _fill(LT, 31), tg, stride, 1)
    return np.stack([trace_mask_for(v), _trace_body(32)])


def trace_extreme_digits():
    """Digits of sign + and -: base-4 balanced digits lie in [-2, 1], so +1 and -2 below the top."""
    return extreme_digits(LT)


def trace_spectral_case(dk):
    _, _, _, m, _ = spectral_peak(LT, dk)
    v = targets_from_signs(LT, aligned_signs(LT.n, m))
    return np.stack([trace_mask_for(v), _trace_body(33)])


def trace_coefficient_case(dk, c):
    _, r, o, _, _ = spectral_peak(LT, dk)
    row = key_step_rows(LT, dk, 0)[r, o]
    j = np.arange(2048)
    s = np.where(j <= c, 1, -1) * np.where(row[(c - j) % 2048] >= 0, 1, -1)
    return np.stack([trace_mask_for(targets_from_signs(LT, s)), _trace_body(34)])


def trace_random_case(seed=78):
    return np.random.default_rng(seed).integers(0, Q2, (2, 2048), dtype=np.uint64)


def trace_aligned_names():
    return ["spectral"] + [f"coef_aligned_{c}" for c in COEF_ALIGNED(LT)]


def trace_cases(dk):
    out = {"boundary": trace_boundary_case(), "spectral": trace_spectral_case(dk)}
    for c in COEF_ALIGNED(LT):
        out[f"coef_aligned_{c}"] = trace_coefficient_case(dk, c)
    out["zero_mask"] = np.stack([np.zeros(2048, dtype=np.uint64), _trace_body(35)])
    out["zero_body"] = np.stack([trace_boundary_case()[0], np.zeros(2048, dtype=np.uint64)])
    return out
