"""Scale spaces with an exactly known number of extrema per octave, for the keypoint stages at their count boundaries
(tests/test_planted.py checks the generator against the oracle, tests/test_gpu_count_edges.py runs the device on it).

Every octave's DoG planes hold isolated paraboloid bumps on a lattice, on a plateau of 0:
    D(x, y, z) = s * max(A - a ((x - xc)^2 + (y - yc)^2) - c (z - zc)^2, 0)        s = +1 (maximum) or -1 (minimum)
with a sub-pixel centre (|xc - x|, |yc - y|, |zc - z| <= 0.3 around lattice pixel (x, y) and search level z).  The
finite differences of a paraboloid are exact, so each bump is one candidate (a strict extremum of its 3 x 3 x 3
neighbourhood, nothing else is: the plateau is flat) and refines to (xc, yc, zc) in one step.  A = 50 passes every
sift mode's contrast tests (2 * threshold = 3.4), the Hessian -2a I passes the edge test (tr^2 / det = 4 < 12.1), and
the support (radius sqrt(A / a) = 3.5) is far inside the lattice spacing, so no two bumps meet in a 3 x 3 x 3 test.

The Gaussian planes (orientation and descriptor input) are a sum of sinusoids with seeded random directions, frequencies
and phases plus a ramp: smooth, without mirror symmetry (so histogram peaks do not tie and orientations can be compared
one by one), different at every level.

The lattice spans the detectable area: its first and last rows and columns are the first and last rows and columns the
detection examines (1 and w - 2, or 5 and w - 6 in OpenCV mode), so orientation windows and descriptor patches there are
clipped by the plane border.  The levels cycle through the whole search range 1 .. levels (`levels` of Planted, the
params' levels: 3 by default, up to 9); with pin_z the first bump on level 1 is centred at zc = 0.7 and the first on the top
search level at zc = levels + 0.3, the outermost sub-level centres refinement accepts.
"""
import numpy as np

A, CURV, ZCURV = 50.0, 4.0, 4.0
SPACING = 10
LEVELS = 3                      # the default params' levels: DoG planes 0 .. 4, search levels 1 .. 3
DOG_PLANES, GAUSS_PLANES = LEVELS + 2, LEVELS + 3
DET_W, DET_RH, DET_SUBQ = 64, 32, 64   # extrema.hip: detection strip width / rows, candidate sub-queues


def border(sift_mode=0):
    """first detectable row / column (x >= 1, or x >= 5 in OpenCV mode, extrema.hip k_detect)"""
    return 5 if sift_mode == 1 else 1


def lattice(w, h, sift_mode=0, rect=None):
    """(x, y) lattice sites of a w x h octave, SPACING apart, first and last detectable row and column included;
    rect = (x0, y0, x1, y1): only the sites inside [x0, x1) x [y0, y1)"""
    b = border(sift_mode)

    def axis(n):
        lo, hi = b, n - 1 - b
        if hi < lo:
            return np.zeros(0, np.int64)
        k = (hi - lo) // SPACING + 1
        return lo + (np.arange(k) * (hi - lo)) // max(k - 1, 1)
    xs, ys = axis(w), axis(h)
    yy, xx = np.meshgrid(ys, xs, indexing="ij")
    pts = np.stack([xx.ravel(), yy.ravel()], 1)
    if rect is not None:
        x0, y0, x1, y1 = rect
        pts = pts[(pts[:, 0] >= x0) & (pts[:, 0] < x1) & (pts[:, 1] >= y0) & (pts[:, 1] < y1)]
    return pts


def capacity(w, h, sift_mode=0, rect=None):
    return len(lattice(w, h, sift_mode, rect))


def subq_rect(w, h, q):
    """the pixels (x0, y0, x1, y1) whose candidates go to detection sub-queue q of a w x h octave: the strip's cell of an
    8 x 8 grid over the octave (extrema.hip k_detect: subq = (cy * 8 / urows) * 8 + sx * 8 / strips)"""
    strips = (w - 2) // DET_W + 1
    urows = (h - 2 + DET_RH - 1) // DET_RH
    qy, qx = divmod(q, 8)
    sx = [s for s in range(strips) if s * 8 // strips == qx]
    cy = [r for r in range(urows) if r * 8 // urows == qy]
    if not sx or not cy:
        return (0, 0, 0, 0)
    return (sx[0] * DET_W, 1 + cy[0] * DET_RH, (sx[-1] + 1) * DET_W, 1 + (cy[-1] + 1) * DET_RH)


def subq_of(w, h, x, y):
    """the detection sub-queue of a candidate at pixel (x, y) of a w x h octave (the inverse of subq_rect)"""
    strips = (w - 2) // DET_W + 1
    urows = (h - 2 + DET_RH - 1) // DET_RH
    return ((np.asarray(y) - 1) // DET_RH * 8 // urows) * 8 + np.asarray(x) // DET_W * 8 // strips


class Planted:
    """dims: [(w, h)] per octave; request: {octave: n} or {octave: (n, rect)}; sites are drawn from the octave's lattice
    (inside rect) by a seeded permutation that puts the four corners and the edges first.  Attributes: dog[o][z],
    gauss[o][z] (float32 planes), bumps[o] (structured: x, y, z pixel and level, xc, yc, zc centre, sign), counts.
    levels: DoG search levels (levels + 2 DoG, levels + 3 Gaussian planes per octave); pin_z: see the module's notes."""

    def __init__(self, dims, request, seed=0, sift_mode=0, minima=True, levels=LEVELS, pin_z=False):
        rng = np.random.default_rng(seed)
        self.levels = levels
        self.dims = list(dims)
        self.counts = [0] * len(self.dims)
        self.bumps, self.dog, self.gauss = [], [], []
        for o, (w, h) in enumerate(self.dims):
            req = request.get(o, 0)
            n, rect = (req, None) if np.isscalar(req) else req
            sites = lattice(w, h, sift_mode, rect)
            if n > len(sites):
                raise ValueError("octave %d (%d x %d): %d extrema requested, the lattice holds %d" % (o, w, h, n, len(sites)))
            b = border(sift_mode)
            edge = (sites[:, 0] == b) | (sites[:, 0] == w - 1 - b) | (sites[:, 1] == b) | (sites[:, 1] == h - 1 - b)
            corner = ((sites[:, 0] == b) | (sites[:, 0] == w - 1 - b)) & ((sites[:, 1] == b) | (sites[:, 1] == h - 1 - b))
            perm = rng.permutation(len(sites))
            order = perm[np.argsort(-(corner[perm].astype(int) + edge[perm].astype(int)), kind="stable")]
            pick = sites[order[:n]]
            bt = np.zeros(n, [("x", np.int32), ("y", np.int32), ("z", np.int32), ("xc", np.float64), ("yc", np.float64),
                              ("zc", np.float64), ("sign", np.int32)])
            bt["x"], bt["y"] = pick[:, 0], pick[:, 1]
            bt["z"] = 1 + (rng.permutation(n) % levels)
            off = rng.uniform(0.05, 0.3, (n, 3)) * rng.choice([-1.0, 1.0], (n, 3))
            if pin_z:
                for z, dz in ((1, -0.3), (levels, 0.3)):
                    at = np.nonzero(bt["z"] == z)[0]
                    if len(at):
                        off[at[0], 2] = dz
            bt["xc"], bt["yc"], bt["zc"] = bt["x"] + off[:, 0], bt["y"] + off[:, 1], bt["z"] + off[:, 2]
            bt["sign"] = rng.choice([-1, 1], n) if minima else 1
            self.bumps.append(bt)
            self.counts[o] = n
            self.dog.append(dog_planes(w, h, bt, levels + 2))
            self.gauss.append(gauss_planes(w, h, rng, planes=levels + 3))

    @classmethod
    def from_tables(cls, dims, tables, seed=0, levels=LEVELS):
        """a Planted from caller-chosen bump tables: tables = {octave: bump_table(...)} (octaves left out are empty).
        Bumps that share a level and a sub-pixel offset triple refine to bit-identical sigmas (the DoG values around
        them are the same numbers), so scale ties of any size can be planted; the Gaussian planes are drawn from `seed`."""
        rng = np.random.default_rng(seed)
        self = cls.__new__(cls)
        self.levels = levels
        self.dims = list(dims)
        self.counts = [0] * len(self.dims)
        self.bumps, self.dog, self.gauss = [], [], []
        for o, (w, h) in enumerate(self.dims):
            bt = np.ascontiguousarray(tables.get(o, np.zeros(0, BUMP_DTYPE)), BUMP_DTYPE)
            if len(bt):
                if len(set(zip(bt["x"].tolist(), bt["y"].tolist()))) != len(bt):
                    raise ValueError("octave %d: two bumps at one site" % o)
                if bt["x"].min() < 1 or bt["x"].max() > w - 2 or bt["y"].min() < 1 or bt["y"].max() > h - 2 or \
                        bt["z"].min() < 1 or bt["z"].max() > levels:
                    raise ValueError("octave %d (%d x %d): a bump outside the detectable volume" % (o, w, h))
            self.bumps.append(bt)
            self.counts[o] = len(bt)
            self.dog.append(dog_planes(w, h, bt, levels + 2))
            self.gauss.append(gauss_planes(w, h, rng, planes=levels + 3))
        return self

    @property
    def total(self):
        return sum(self.counts)

    def load_oracle(self, orc):
        """overwrite the planes of an oracle that has run on a zero image of the planted size; redo its keypoint stages"""
        self._check_dims(orc.num_octaves, orc.octave_dims)
        for o in range(len(self.dims)):
            for z, p in enumerate(self.dog[o]):
                orc.plane(o, 1, z, copy=False)[:] = p
            for z, p in enumerate(self.gauss[o]):
                orc.plane(o, 0, z, copy=False)[:] = p
        return orc.run_keypoint_stages()

    def upload(self, ctx):
        """upload the planes into a store_dog = 1 Context that has run on a zero image of the planted size"""
        self._check_dims(ctx.report().num_octaves, ctx.octave_dims)
        for o in range(len(self.dims)):
            for z, p in enumerate(self.dog[o]):
                ctx.upload_plane(o, 1, z, p)
            for z, p in enumerate(self.gauss[o]):
                ctx.upload_plane(o, 0, z, p)
        return ctx

    def _check_dims(self, n_oct, octave_dims):
        got = [tuple(octave_dims(o)) for o in range(n_oct)]
        if got != [tuple(d) for d in self.dims]:
            raise ValueError("planted for octaves %s, the target has %s" % (self.dims, got))


BUMP_DTYPE = np.dtype([("x", np.int32), ("y", np.int32), ("z", np.int32), ("xc", np.float64), ("yc", np.float64),
                       ("zc", np.float64), ("sign", np.int32)])


def bump_table(x, y, z, off, sign=1):
    """bumps[o] of a Planted from sites (x, y), levels z, sub-pixel offsets off = (n, 3) (dx, dy, dz) and signs"""
    bt = np.zeros(len(x), BUMP_DTYPE)
    off = np.asarray(off, np.float64).reshape(len(x), 3)
    bt["x"], bt["y"], bt["z"], bt["sign"] = x, y, z, sign
    bt["xc"], bt["yc"], bt["zc"] = bt["x"] + off[:, 0], bt["y"] + off[:, 1], bt["z"] + off[:, 2]
    return bt


def cell_sites(w, h, grid, sift_mode=0, reach=0.31):
    """the lattice sites of a w x h octave with the grid filter's cell of each (tests/filter_rule.py cell_of) and
    `inside`: the whole box of +-reach pixels around the site lies in that one cell, so a bump planted there with
    offsets up to 0.3 is counted in it wherever its centre falls.  Structured: x, y, cell, inside."""
    from filter_rule import cell_of
    pts = lattice(w, h, sift_mode)
    out = np.zeros(len(pts), [("x", np.int32), ("y", np.int32), ("cell", np.int32), ("inside", bool)])
    out["x"], out["y"] = pts[:, 0], pts[:, 1]
    out["cell"] = cell_of(out["x"], out["y"], w, h, grid)
    out["inside"] = True
    for dx in (-reach, reach):
        for dy in (-reach, reach):
            out["inside"] &= cell_of(out["x"] + dx, out["y"] + dy, w, h, grid) == out["cell"]
    return out


def dog_planes(w, h, bumps, n_planes=DOG_PLANES):
    out = np.zeros((n_planes, h, w), np.float64)
    r = int(np.ceil(np.sqrt(A / CURV))) + 1
    for b in bumps:
        x0, x1 = max(b["x"] - r, 0), min(b["x"] + r + 1, w)
        y0, y1 = max(b["y"] - r, 0), min(b["y"] + r + 1, h)
        yy, xx = np.mgrid[y0:y1, x0:x1].astype(np.float64)
        d2 = (xx - b["xc"]) ** 2 + (yy - b["yc"]) ** 2
        for z in range(n_planes):
            v = np.maximum(A - CURV * d2 - ZCURV * (z - b["zc"]) ** 2, 0.0)
            out[z, y0:y1, x0:x1] += b["sign"] * v
    return [p.astype(np.float32) for p in out]


def gauss_planes(w, h, rng, terms=5, planes=GAUSS_PLANES):
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    out = []
    ramp = rng.uniform(-0.05, 0.05, 2)
    th = rng.uniform(0, 2 * np.pi, terms)
    fr = rng.uniform(0.05, 0.35, terms)
    am = rng.uniform(4.0, 12.0, terms)
    for z in range(planes):
        g = 100.0 + ramp[0] * xx + ramp[1] * yy
        for k in range(terms):
            ph = rng.uniform(0, 2 * np.pi)
            g += am[k] * np.sin(fr[k] * (np.cos(th[k] + 0.05 * z) * xx + np.sin(th[k] + 0.05 * z) * yy) + ph)
        out.append(g.astype(np.float32))
    return out


def params_kw(octaves, **kw):
    """the params of a planted case: no upscaling (octave 0 is the image), `octaves` octaves, the default levels unless
    kw names others"""
    d = dict(upscale_factor=0.0, octaves=octaves, levels=LEVELS)
    d.update(kw)
    return d


def octave_dims(O, w, h, octaves, **kw):
    """the octave sizes of a w x h image under params_kw (from the oracle: no GPU needed)"""
    orc = O.Oracle(O.default_params(**params_kw(octaves, **kw)), threads=1).run(np.zeros((h, w), np.uint8), keypoints=False)
    return [orc.octave_dims(o) for o in range(orc.num_octaves)]
