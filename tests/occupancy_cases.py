"""Constructed rays, bitmaps and clouds for cg_occupancy_set_bits / cg_occupancy_grid_rays (csrc/occupancy.hip), one cause each.

Leaves and queries are given in units of the resolution: a leaf by its integer key (key - 32768 per axis), a query by a multiple of
0.5.  At RES = 2^-10 leaf centres (k + 0.5) RES and queries are exact float32 numbers; RES_MM = 0.001f repeats the ray cases
without that claim.  The reference of one ray is oracle.collision_oracle.cast_ray over points at the leaf centres, followed by the keep
rule of cr_make_occupancy_grid restated here in float32 (`direction`, `keep_rule`); tests/test_occupancy_cases_cpu.py proves the
restatement equal to cr_make_occupancy_grid itself, then certifies every case below against it.

`Ray.hit` / `Ray.end` / `Ray.keep` are the constructed outcome (end: the key of the leaf the ray stops in), `Ray.cause` what decides it."""
import numpy as np

RES = np.float32(2.0 ** -10)
RES_MM = np.float32(0.001)
RANGE = 64.0            # default max_range in units of the resolution: a missing ray ends after ~64 steps
PAD = np.float32(0.005)


class Ray:
    def __init__(self, name, cause, leaves, q, hit, end=None, keep=False, max_range=RANGE):
        self.name, self.cause, self.leaves, self.q = name, cause, [tuple(l) for l in leaves], tuple(float(v) for v in q)
        self.hit, self.end, self.keep, self.max_range = hit, None if end is None else tuple(end), keep, max_range

    def __repr__(self):
        return self.name

    def query(self, res):
        return (np.array(self.q, dtype=np.float64) * np.float64(res)).astype(np.float32)

    def range(self, res):
        """max_range as the float the reference passes (0 = disabled); a Ray may carry an exact float32 instead of units (`abs_range`)"""
        if getattr(self, 'abs_range', None) is not None:
            return np.float32(self.abs_range)
        return np.float32(np.float64(self.max_range) * np.float64(res))


def centres(leaves, res):
    """(n,3) float32 leaf centres, as the kernel and the oracle compute them: (float)((k + 0.5) * (double)res)"""
    k = np.asarray(leaves, dtype=np.float64).reshape(-1, 3)
    return ((k + 0.5) * np.float64(np.float32(res))).astype(np.float32)


def direction(q):
    """cr_make_occupancy_grid: dir = q / sqrtf((x x + y y) + z z), q itself when that is 0"""
    x, y, z = (np.float32(v) for v in q)
    sq = np.float32(np.float32(x * x + y * y) + z * z)
    if sq > 0:
        nrm = np.sqrt(sq, dtype=np.float32)
        return np.array([x / nrm, y / nrm, z / nrm], dtype=np.float32)
    return np.array([x, y, z], dtype=np.float32)


def keep_rule(q, hit, end):
    """kept iff hit and (float)sqrt((double)(end . end)) <= sqrtf(q . q), both dot products summed left to right in float"""
    if not hit:
        return False
    x, y, z = (np.float32(v) for v in q)
    e0, e1, e2 = (np.float32(v) for v in end)
    dist_query = np.sqrt(np.float32(np.float32(x * x + y * y) + z * z), dtype=np.float32)
    dist = np.float32(np.sqrt(np.float64(np.float32(np.float32(e0 * e0 + e1 * e1) + e2 * e2))))
    return bool(dist <= dist_query)


def lattice_of(pts, res):
    """my_cpp/common.cpp:353-376 in float32 -> origin (3,), counts (3,), max_range (float32)"""
    a = np.ascontiguousarray(pts, dtype=np.float32); res = np.float32(res)
    mx, mn = a.max(axis=0), a.min(axis=0)
    n = [int(np.float32(np.float32(np.float32(mx[i] + PAD) - np.float32(mn[i] - PAD)) / res)) for i in range(3)]
    origin = np.array([np.float32(mn[i] - PAD) for i in range(3)], dtype=np.float32)
    max_range = np.float32(np.sqrt(sum(float(np.float32(mx[i] + PAD)) ** 2 for i in range(3))))
    return origin, n, max_range


def lattice_points(origin, n, res):
    """(nx ny nz, 3) float32, x slowest: o + i * res, product and sum each rounded to float"""
    res = np.float32(res)
    ax = [np.float32(origin[i]) + np.arange(n[i], dtype=np.float32) * res for i in range(3)]
    return np.stack(np.meshgrid(*ax, indexing='ij'), axis=-1).reshape(-1, 3).astype(np.float32)


# ---- 1. tie order ------------------------------------------------------------------------------------------------------------------
def tie_cases():
    out = []
    a = 8
    # (+,+,+): all three tMax equal at every corner of the diagonal; `<` takes z, then y, then x
    for leaf, hit in (((0, 0, 1), True), ((0, 1, 1), True), ((1, 1, 1), True), ((1, 0, 0), False), ((0, 1, 0), False), ((1, 0, 1), False),
                      ((1, 1, 0), False)):
        out.append(Ray(f'tie-ppp-leaf{leaf}', 'tie order z, y, x', [leaf], (a, a, a), hit, leaf if hit else None, hit))
    # a negative component starts with tMax = 0: the origin sits on that face of its leaf.  The walk leaves the origin leaf once, so exactly
    # one of the three axis neighbours is ever entered: z's if z < 0, else y's if y < 0, else x's; all positive: z's (above)
    for sx in (1, -1):
        for sy in (1, -1):
            for sz in (1, -1):
                first = 2 if sz < 0 else 1 if sy < 0 else 0 if sx < 0 else 2
                for axis, s in enumerate((sx, sy, sz)):
                    leaf = [0, 0, 0]; leaf[axis] = s
                    hit = axis == first
                    out.append(Ray(f'tie-octant{sx:+d}{sy:+d}{sz:+d}-axis{axis}', 'first neighbour', [leaf], (sx * a, sy * a, sz * a), hit,
                                   leaf if hit else None, hit))
    for q, first, other in (((a, a, 0), (0, 1, 0), (1, 0, 0)), ((a, 0, a), (0, 0, 1), (1, 0, 0)), ((0, a, a), (0, 0, 1), (0, 1, 0))):
        out.append(Ray(f'tie-face{q}-first', 'face diagonal', [first], q, True, first, True))
        out.append(Ray(f'tie-face{q}-other', 'face diagonal', [other], q, False))
    return out


# ---- 2. zero components, 3. origin leaf, 4. keep rule --------------------------------------------------------------------------------
def zero_component_cases():
    out = []
    for axis in range(3):
        for s in (1, -1):
            q = [0, 0, 0]; q[axis] = 8 * s
            on = [0, 0, 0]; on[axis] = 3 * s         # a leaf of the axis column
            off = list(on); off[(axis + 1) % 3] = 1                    # its neighbour across a face the ray never crosses
            off2 = list(on); off2[(axis + 2) % 3] = -1
            out.append(Ray(f'axis{axis}{s:+d}-column', 'two zero steps', [on], q, True, on, True))
            out.append(Ray(f'axis{axis}{s:+d}-beside', 'two zero steps', [off, off2], q, False))
    out.append(Ray('zero-query-free-origin', 'no direction', [(0, 0, 1), (1, 0, 0), (-1, -1, -1)], (0, 0, 0), False))
    out.append(Ray('zero-query-occupied-origin', 'dist_query = 0', [(0, 0, 0)], (0, 0, 0), True, (0, 0, 0), False))
    return out


def origin_leaf_cases():
    out = [Ray('origin-leaf-q(1,0,0)', 'origin leaf', [(0, 0, 0), (1, 0, 0)], (1, 0, 0), True, (0, 0, 0), True),
           Ray('origin-leaf-q-at-centre', 'keep at equality', [(0, 0, 0)], (0.5, 0.5, 0.5), True, (0, 0, 0), True),
           Ray('origin-leaf-q-short', 'keep rule', [(0, 0, 0)], (0.5, 0.5, 0), True, (0, 0, 0), False)]
    for q in ((-8, 3, 5), (0, 0, -9), (7, -7, 7)):
        out.append(Ray(f'origin-leaf-q{q}', 'origin leaf', [(0, 0, 0), (0, 0, -1), (1, 0, 0)], q, True, (0, 0, 0), True))
    return out


LEAF20 = (0, 0, 20)       # centre (0.5, 0.5, 20.5): distance sqrt(420.75) = 20.512...


def keep_rule_cases():
    return [Ray(f'keep-z{z}', 'dist <= dist_query', [LEAF20], (0, 0, z), True, LEAF20, z >= 21, max_range=0) for z in (19, 20, 21, 22)]


# ---- 5. max_range ------------------------------------------------------------------------------------------------------------------
def range_brackets(res):
    """the two neighbouring floats r_lo < r_hi with r_lo^2 < dsq <= r_hi^2 for LEAF20's centre, by the kernel's own rule (float64 sum of
    the squared float centre coordinates against max_range^2).  dsq == r^2 is unreachable through leaf centres: in units of res / 2 the
    squared distance is a sum of three odd squares, = 3 mod 8, and no integer square is; and a float r with that r^2 would have to be
    such an integer multiple."""
    c = centres([LEAF20], res)[0].astype(np.float64)
    dsq = c[0] * c[0] + c[1] * c[1] + c[2] * c[2]
    r = np.float32(np.sqrt(dsq))
    while np.float64(r) * np.float64(r) >= dsq:
        r = np.nextafter(r, np.float32(0))
    hi = np.nextafter(r, np.float32(np.inf))
    assert np.float64(r) ** 2 < dsq < np.float64(hi) ** 2
    return r, hi


def range_cases(res):
    q = (0, 0, 22)
    lo, hi = range_brackets(res)
    out = [Ray('range-20.5', 'range before occupancy', [LEAF20], q, False, max_range=20.5),
           Ray('range-disabled', 'max_range = 0', [LEAF20], q, True, LEAF20, True, max_range=0),
           Ray('range-float-below', 'dsq > max_range^2', [LEAF20], q, False),
           Ray('range-float-above', 'dsq > max_range^2', [LEAF20], q, True, LEAF20, True)]
    out[2].abs_range, out[3].abs_range = lo, hi
    return out


# ---- 6. key border -----------------------------------------------------------------------------------------------------------------
def border_cases():
    out = []
    for axis in range(3):
        for s in (1, -1):
            q = [0, 0, 0]; q[axis] = 8 * s
            out.append(Ray(f'border-axis{axis}{s:+d}', 'key border', [], q, False, max_range=0))
    out.append(Ray('border-diagonal', 'key border', [], (8, -8, 8), False, max_range=0))
    return out


# ---- 7. bitmap addressing ----------------------------------------------------------------------------------------------------------
DIMS = (3, 5, 7)
OFFSET = (-2, 3, 17)


def bit_index(key, offset=OFFSET, dims=DIMS):
    ix, iy, iz = (key[a] - offset[a] for a in range(3))
    assert 0 <= ix < dims[0] and 0 <= iy < dims[1] and 0 <= iz < dims[2]
    return (ix * dims[1] + iy) * dims[2] + iz


def key_of_bit(i, offset=OFFSET, dims=DIMS):
    return (i // (dims[1] * dims[2]) + offset[0], (i // dims[2]) % dims[1] + offset[1], i % dims[2] + offset[2])


def pack(keys, offset=OFFSET, dims=DIMS):
    """the bitmap words of a key list, packed by numpy: bit i of the box in word i >> 5 at position i & 31"""
    n = dims[0] * dims[1] * dims[2]
    bits = np.zeros(((n + 31) // 32) * 32, dtype=np.uint8)
    for k in keys:
        bits[bit_index(k, offset, dims)] = 1
    return np.packbits(bits.reshape(-1, 32), axis=1, bitorder='little').view('<u4').reshape(-1)


def corners(offset=OFFSET, dims=DIMS):
    return [(offset[0] + i * (dims[0] - 1), offset[1] + j * (dims[1] - 1), offset[2] + k * (dims[2] - 1)) for i in (0, 1) for j in (0, 1) for k in (0, 1)]


class BoxRay(Ray):
    """a ray against a hand-placed key box: `offset` the box corner, `leaves` the set bits (all inside the box), `ghost` the cell outside
    the box the ray does pass through, next to the set bit: occupied instead, it is hit (the CPU certificate of adjacency)"""

    def __init__(self, name, offset, leaves, ghost, q):
        super().__init__(name, 'out-of-box lookup', leaves, q, False)
        self.offset, self.ghost = offset, ghost


def box_face_cases():
    """the ray runs along index -1 or index d of the box, past a set bit in the adjacent in-box cell, and must not see it"""
    out = []
    z = (0, 0, 40)          # +z ray: cells (0, 0, k)
    x = (40, 0, 0)          # +x ray: cells (k, 0, 0)
    out.append(BoxRay('box-face-x-low', (1, -2, 17), [(1, 0, 20)], (0, 0, 20), z))              # ix = -1
    out.append(BoxRay('box-face-x-high', (-3, -2, 17), [(-1, 0, 20)], (0, 0, 20), z))           # ix = 3 = dx
    out.append(BoxRay('box-face-y-low', (-1, 1, 17), [(0, 1, 20)], (0, 0, 20), z))              # iy = -1
    out.append(BoxRay('box-face-y-high', (-1, -5, 17), [(0, -1, 20)], (0, 0, 20), z))           # iy = 5 = dy
    out.append(BoxRay('box-face-z-low', (19, -2, 1), [(20, 0, 1)], (20, 0, 0), x))              # iz = -1
    out.append(BoxRay('box-face-z-high', (19, -2, -7), [(20, 0, -1)], (20, 0, 0), x))           # iz = 7 = dz
    # through the box and out of its y-high face: y = z / 4, so the ray is inside the box (y <= 1) up to z = 8 and at iy = 5 = dy after
    out.append(BoxRay('box-exit-y-high', (-1, -3, 3), [(0, 1, 9)], (0, 2, 9), (0, 8, 32)))
    return out


# ---- 8. lattice --------------------------------------------------------------------------------------------------------------------
LATTICE_N = (7, 5, 11)
LATTICE_ORIGIN = (-3, -2, -5)          # in units of the resolution: lattice point (3, 2, 5) is q = 0 exactly
LATTICE_LEAVES = [(0, 0, 2), (-1, 0, 1), (1, -1, -2), (-2, 1, 0), (0, -1, 0), (2, 1, 4)]


# ---- 9. wrapper clouds -------------------------------------------------------------------------------------------------------------
def cloud_axis_patch():
    """(a) a bumpy patch centred on the optical axis: x, y of both signs and exactly 0"""
    g = np.arange(-4, 5) * 0.002
    x, y = np.meshgrid(g, g, indexing='ij')
    z = 0.3 + 0.004 * np.cos(400.0 * x) * np.cos(300.0 * y)
    return np.stack([x, y, z], axis=-1).reshape(-1, 3).astype(np.float32), np.float32(0.002)


def cloud_origin_leaf():
    """(b) a point inside the origin's leaf, in front of a small wall"""
    g = np.arange(0, 6) * 0.001
    x, y = np.meshgrid(g - 0.002, g - 0.003, indexing='ij')
    wall = np.stack([x, y, np.full_like(x, 0.006)], axis=-1).reshape(-1, 3)
    return np.concatenate([[[0.0004, 0.0006, 0.0002]], wall]).astype(np.float32), np.float32(0.001)


def cloud_integer_extent():
    """(c) RES = 2^-10; x = +-mx with fl(mx + pad) = 26 * 2^-11 exactly, so the padded x extent / res is the integer 26 in float
    arithmetic: the (int) truncation sits on its edge"""
    target = np.float32(26 * 2.0 ** -11)
    mx = np.float32(target - PAD)
    assert np.float32(mx + PAD) == target
    rng = np.random.default_rng(7)
    pts = np.stack([rng.uniform(-float(mx), float(mx), 60), rng.uniform(-0.004, 0.004, 60), rng.uniform(0.05, 0.056, 60)], axis=1)
    pts[0, 0], pts[1, 0] = mx, -mx
    return pts.astype(np.float32), RES


CLOUDS = {'axis-patch': cloud_axis_patch, 'origin-leaf': cloud_origin_leaf, 'integer-extent': cloud_integer_extent}


def ray_cases(res):
    return tie_cases() + zero_component_cases() + origin_leaf_cases() + keep_rule_cases() + range_cases(res)
