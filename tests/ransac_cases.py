"""Constructed hypotheses for cg_ransac_9d / cg_similarity_inliers (csrc/ransac.hip), one cause each.

The exact family: the sample is the tetrahedron 0.25 * {0, e1, e2, e3} (cloud rows 0..3), the model dst = A0 src + T0 with
A0 = PCYC diag(0.5, 0.25, 0.125), PCYC the cyclic permutation matrix (det +1), T0 dyadic, threshold 2^-8.  Every number is a
dyadic rational of a few bits, so the 4 x 7 elimination, the column norms, the Gram matrix (exactly I: Jacobi does nothing), the
nearest rotation, the inverse, the canonical coordinates and the residuals are computed without rounding, by the kernel and by the
oracle alike (tests/test_ransac_cases_cpu.py asserts it for the oracle).  A comparison that sits exactly ON a bound is therefore
decided by the comparison operator alone.

The shear family (singular-value gate) is not exact; its singular values keep >= 1e-3 from 0.8 and 1.2 (SIGMA_MARGIN) because the
kernel's Jacobi and LAPACK differ in the last bits.

Every case is ONE hypothesis (H = 1) except `orderings()`; `Case.accept` / `Case.count` are the constructed verdict, `Case.cause`
names the only gate that can reject it, `Case.relaxed()` is the same input with only that bound opened (None where the gate has no
bound to open: singular values, determinant, degeneracy).  SAMPLES collects every 4-point sample any case uses."""
import itertools

import numpy as np

THRES = 2.0 ** -8
S3 = np.array([0.5, 0.25, 0.125])
PCYC = np.array([[0.0, 0.0, 1.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])
A0 = PCYC @ np.diag(S3)
T0 = np.array([0.5, -0.25, 1.0])
TETRA = 0.25 * np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]])
OPEN_MIN, OPEN_MAX = np.zeros(3), np.full(3, 99.0)
WIDE_DIMS = 4.0
SIGMA_MARGIN = 1e-3
# T of an accepted hypothesis, device against oracle, where the arithmetic is not exact (shear cases, the random cloud of
# tests/test_aligning_gpu.py): 16 x the larger of two gaps, both the largest |dT| entry over all accepted hypotheses of that test's 600:
#   ORACLE_LD_GAP  the oracle (float64, LAPACK) against the same formulas in np.longdouble; test_ransac_cases_cpu.py recomputes it
#   DEVICE_GAP     the device against the oracle, measured on an MI355X; test_aligning_gpu.py prints it
# The factor 16 leaves room for another, equally valid, operation order.
ORACLE_LD_GAP = 4.341e-15
DEVICE_GAP = 5.441e-15
T_TOL = 16 * max(ORACLE_LD_GAP, DEVICE_GAP)

NS = (4, 5, 64, 65, 255, 256, 257, 600)
_PS = (4, 63, 64, 127, 128, 191, 192, 255, 256, 511)

SAMPLES = []           # (name, (4,3) src rows) of every sample used by a case


def positions(N):
    """witness rows for a cloud of N: each of the four waves, lane 0 and lane 63, the second stride, the ragged tail"""
    return sorted({p for p in _PS + (N - 1,) if 4 <= p < N})


def filler(N):
    """(N,3) source cloud: the tetrahedron, then dyadic points inside its extent [0, 0.25]^3"""
    p = np.arange(N)
    src = np.stack([(p * 5) % 17, (p * 7) % 17, (p * 11) % 17], axis=1) / 64.0
    src[:4] = TETRA
    return src


def model(src, A=A0, t=T0):
    return src @ A.T + t


def mat4(A, t):
    T = np.eye(4); T[:3, :3] = A; T[:3, 3] = t
    return T


class Case:
    def __init__(self, name, cause, src, dst, accept, count=None, ids=None, T=None, exact=True, min_scale=OPEN_MIN, max_scale=OPEN_MAX,
                 max_dims=None, thres=THRES, relax=None):
        self.name, self.cause, self.exact, self.thres, self.relax = name, cause, exact, thres, relax
        self.src, self.dst = np.ascontiguousarray(src, dtype=np.float64), np.ascontiguousarray(dst, dtype=np.float64)
        self.ids = np.ascontiguousarray([[0, 1, 2, 3]] if ids is None else ids, dtype=np.int32).reshape(-1, 4)
        self.accept = np.broadcast_to(np.asarray(accept, dtype=bool), (len(self.ids),)).copy()
        self.count = None if count is None else np.where(self.accept, count, -1).astype(np.int32)    # None: the oracle's
        self.T = T                                                   # expected 4x4 of the accepted rows (None: the oracle's)
        self.min_scale, self.max_scale = np.array(min_scale, dtype=np.float64), np.array(max_scale, dtype=np.float64)
        self.max_dims = None if max_dims is None else np.array(max_dims, dtype=np.float64)
        for row in self.ids:
            SAMPLES.append((name, self.src[row]))

    @property
    def N(self):
        return len(self.src)

    def relaxed(self):
        """the same input with only the named bound opened, or None"""
        if self.relax is None:
            return None
        c = Case.__new__(Case)
        c.__dict__.update(self.__dict__)
        c.name = self.name + '-relaxed'
        for k, v in self.relax.items():
            setattr(c, k, v)
        c.accept = np.ones_like(self.accept); c.count = None
        return c

    def __repr__(self):
        return self.name


def _exact_cloud(N=8):
    src = filler(N)
    return src, model(src)


# ---- 1. scale bounds ---------------------------------------------------------------------------------------------------------------
def scale_cases():
    out = []
    src, dst = _exact_cloud()
    for j in range(3):
        for side in ('max', 'min'):
            for on in (True, False):
                b = (OPEN_MAX if side == 'max' else OPEN_MIN).copy()
                b[j] = S3[j] if on else np.nextafter(S3[j], 0.0 if side == 'max' else 1.0)
                kw = {f'{side}_scale': b}
                out.append(Case(f'scale-{side}{j}-{"on" if on else "past"}', f'{side}_scale[{j}]', src, dst, on, count=len(src),
                                T=mat4(A0, T0), relax=None if on else {f'{side}_scale': OPEN_MAX if side == 'max' else OPEN_MIN}, **kw))
    return out


# ---- 2. singular values ------------------------------------------------------------------------------------------------------------
def shear_matrix(kind, c):
    """unit columns: 'two' -> columns 0 and 1 at cosine c, column 2 orthogonal (sigma = sqrt(1 +- c), 1);
    'three' -> all pairs at cosine c (sigma = sqrt(1 + 2c), sqrt(1 - c) twice)"""
    if kind == 'two':
        return np.array([[1.0, c, 0.0], [0.0, np.sqrt(1.0 - c * c), 0.0], [0.0, 0.0, 1.0]])
    return np.linalg.cholesky(np.array([[1.0, c, c], [c, 1.0, c], [c, c, 1.0]])).T


def shear_sigmas(kind, c):
    return (np.sqrt(1 - c), np.sqrt(1 + c)) if kind == 'two' else (np.sqrt(1 - c), np.sqrt(1 + 2 * c))


SHEARS = (('two', 0.35, True, None), ('two', 0.40, False, 'sigma_min'), ('three', 0.20, True, None), ('three', 0.30, False, 'sigma_max'))


def shear_cases():
    out = []
    src = filler(8)
    for kind, c, ok, cause in SHEARS:
        A = shear_matrix(kind, c) @ np.diag(S3)
        dst = model(src, A)
        # the returned T is the nearest rotation x scales, not A: the sample rows themselves miss by 4e-3 .. 2e-2.  The other rows are
        # moved far away and the threshold is 2^-10, so that no residual is within a factor 2 of it
        dst[4:] += 1.0
        out.append(Case(f'shear-{kind}-{c:.2f}', cause or 'none', src, dst, ok, exact=False, thres=2.0 ** -10))
    return out


# ---- 3. reflection -----------------------------------------------------------------------------------------------------------------
def reflection_cases():
    src = filler(8)
    mirror = np.diag([1.0, 1.0, -1.0])
    swap = np.array([[0.0, 1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])            # det -1
    swap_pos = np.array([[0.0, 1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, -1.0]])       # det +1
    out = []
    for name, Q, ok in (('mirror', mirror, False), ('swap-neg', swap, False), ('swap-pos', swap_pos, True)):
        A = Q @ np.diag(S3)
        out.append(Case(f'reflect-{name}', 'none' if ok else 'det', src, model(src, A), ok, count=len(src), T=mat4(A, T0)))
    return out


# ---- 4. extent ---------------------------------------------------------------------------------------------------------------------
EXTENT = 0.5            # the cloud's canonical extent on the witness axis: 0 .. 0.5 (end 'max') or -0.25 .. 0.25 (end 'min')


def extent_cloud(N, p, axis, end, witness=True):
    src = filler(N)
    if witness:
        src[p] = 0.125
        src[p, axis] = 0.5 if end == 'max' else -0.25
    return src, model(src)


def extent_cases(N, p, axis, end, witness=True):
    """-> [on the bound (accepted: `>` is strict), just past it (rejected), no bound (accepted)]"""
    src, dst = extent_cloud(N, p, axis, end, witness)
    on = np.full(3, WIDE_DIMS); on[axis] = EXTENT
    past = on.copy(); past[axis] = np.nextafter(EXTENT, 0.0)
    tag = f'extent-N{N}-p{p}-ax{axis}-{end}'
    return [Case(tag + '-on', 'none', src, dst, True, count=N, T=mat4(A0, T0), max_dims=on),
            Case(tag + '-past', f'max_dimensions[{axis}]', src, dst, not witness, count=N, T=mat4(A0, T0), max_dims=past, relax={'max_dims': on}),
            Case(tag + '-nobound', 'none', src, dst, True, count=N, T=mat4(A0, T0), max_dims=None)]


# ---- 5. inlier count ---------------------------------------------------------------------------------------------------------------
OUTLIER = 2.0 ** -2
JUST_ABOVE = THRES * (1.0 + 2.0 ** -40)


def inlier_case(N, p, above):
    """every non-sample row an outlier by 2^-2; row p off by exactly the threshold (counted) or by thres (1 + 2^-40) (not counted)"""
    src = filler(N); dst = model(src)
    q = np.arange(4, N)
    dst[q, q % 3] += OUTLIER
    dst[p, p % 3] -= OUTLIER
    dst[p, p % 3] += (-1.0) ** p * (JUST_ABOVE if above else THRES)
    return Case(f'inlier-N{N}-p{p}-{"above" if above else "on"}', 'threshold', src, dst, True, count=4 if above else 5, T=mat4(A0, T0))


def all_inliers_case(N):
    src = filler(N)
    return Case(f'inlier-N{N}-all', 'none', src, model(src), True, count=N, T=mat4(A0, T0))


# ---- 6. elimination ----------------------------------------------------------------------------------------------------------------
def orderings(N=8):
    src, dst = _exact_cloud(N)
    return Case('orderings', 'none', src, dst, True, count=N, ids=list(itertools.permutations(range(4))), T=mat4(A0, T0))


def degenerate_cases():
    """exactly singular samples -> count -1, 16 zeros.  Rows 4, 5 of the cloud: 0.25 (e1 + e2) (coplanar with 0, e1, e2) and 0.125 e1
    (collinear with 0, e1).  `shift` moves the whole source cloud so that no column of the system is zero and the pivots' inverses round:
    the last pivot is then a rounding residue, not 0, and the RELATIVE criterion has to reject it."""
    out = []
    for shift in (np.zeros(3), np.array([1.0, 2.0, 0.5])):
        src = filler(8)
        src[4] = [0.25, 0.25, 0.0]; src[5] = [0.125, 0.0, 0.0]
        dst = model(src)
        src = src + shift
        s = '' if not shift.any() else '-shifted'
        for name, ids in (('repeated', [0, 1, 1, 2]), ('collinear', [0, 1, 5, 3]), ('coplanar', [0, 1, 2, 4])):
            out.append(Case(f'degenerate-{name}{s}', 'degenerate', src, dst, False, ids=[ids]))
    return out


# ---- 8. cg_similarity_inliers ------------------------------------------------------------------------------------------------------
def mask_case(N):
    """-> src, dst, T (4x4), expected mask: rows cycle through exact inlier (1), error == threshold (1), error just above (0), far (0)"""
    src = filler(N + 4)[4:] if N < 4 else filler(N)
    dst = model(src)
    r = np.arange(N)
    off = np.choose(r % 4, [0.0, THRES, JUST_ABOVE, OUTLIER]) * (-1.0) ** (r // 4)
    dst[r, r % 3] += off
    return src, dst, mat4(A0, T0), (r % 4 < 2).astype(np.uint8)


# ---- 9. selection ------------------------------------------------------------------------------------------------------------------
T1 = np.array([-1.0, 0.5, 2.0])


def selection_cloud(extra_a=3, extra_b=3, extra_c=1):
    """rows 0..3 tetrahedron under model a (T0), 4..7 the tetrahedron again under model b (T1), 8..11 under model c (T0 + 8), then
    extra_a / extra_b / extra_c further rows of each model.  A model's count is 4 + its extras."""
    ta, tb, tc = T0, T1, T0 + 8.0
    n = 12 + extra_a + extra_b + extra_c
    src = filler(n)
    src[4:8] = TETRA; src[8:12] = TETRA
    ts = [ta] * 4 + [tb] * 4 + [tc] * 4 + [ta] * extra_a + [tb] * extra_b + [tc] * extra_c
    dst = np.stack([A0 @ s + t for s, t in zip(src, ts)])
    return src, dst, {'a': ([0, 1, 2, 3], mat4(A0, ta), 4 + extra_a), 'b': ([4, 5, 6, 7], mat4(A0, tb), 4 + extra_b),
                      'c': ([8, 9, 10, 11], mat4(A0, tc), 4 + extra_c), 'bad': ([0, 1, 1, 2], None, -1)}
