"""The inputs that tests/test_gpu_keypoint_teacher.py gives the two keypoint kernels, as numpy arrays built once and never
written.  tests/test_host_keypoint_teacher.py runs them through the oracle alone and checks that they cover what the GPU
comparison is meant to see, so that it cannot pass on empty tables.

Shapes: B = 3 images, K = 70 rows (one past a chunk of 64), a 24 x 16 map, J in {1, 4, 17}."""
import numpy as np

F = np.float32
D = np.float64
B, K, C = 3, 70, 3
MAP_H, MAP_W = 16, 24
JOINTS = (1, 4, 17)
THRESHOLDS = F([0.3, 0.5, 0.4])
MIN_SIZE = 2.0
LONE = 37                       # the one surviving row of image 1
_CACHE = {}


def _frozen(key, make):
    if key not in _CACHE:
        value = make()
        for a in (value.values() if isinstance(value, dict) else value if isinstance(value, tuple) else (value,)):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _CACHE[key] = value
    return _CACHE[key]


def flip_perm(J):
    """The non-trivial permutation of a case: neighbouring joints change places (COCO's pairs for J = 17, joint 0 stays);
    J = 1 has only the identity."""
    perm = np.arange(J, dtype=np.int32)
    for a in range(1 if J % 2 else 0, J - 1, 2):
        perm[a], perm[a + 1] = a + 1, a
    return perm


# ---------------------------------------------------------------------------------------------------------------------
# stage 1: a decoded detection table and its joints
# ---------------------------------------------------------------------------------------------------------------------
def dets(rotated, full=False):
    """[B, K, 6 | 7] float32.  Image 0: no row reaches its threshold.  Image 1: row LONE alone does.  Image 2: about half
    the rows do (rows 65 and 68 among them, row 67 not), some of those are too small, one has a class that is no integer,
    one a NaN edge, one an infinite one (`full`: every row of image 2 survives).  No score within 1e-3 of its threshold,
    no extent within 1e-3 of MIN_SIZE."""
    def make():
        rs = np.random.RandomState(11 + rotated)
        cx, cy = rs.uniform(1, MAP_W - 1, (B, K)), rs.uniform(1, MAP_H - 1, (B, K))
        w, h = rs.uniform(0.6, 8, (B, K)), rs.uniform(0.6, 8, (B, K))
        for e in (w, h):
            e[np.abs(e - MIN_SIZE) < 0.05] = MIN_SIZE + 0.5
        cls = rs.randint(0, C, (B, K))
        score = rs.uniform(0.05, 0.95, (B, K))
        near = np.abs(score - THRESHOLDS[cls]) < 0.01
        score[near] += 0.05
        score[0] = 0.01
        score[1] = 0.02
        score[1, LONE], w[1, LONE], h[1, LONE] = 0.9, 5.0, 4.0
        for k in (65, 68):                                      # survivors past the first chunk of 64 rows, and a drop
            score[2, k], w[2, k], h[2, k] = 0.93, 4.0, 3.0
        score[2, 67] = 0.02
        if full:
            score[2], w[2], h[2] = 0.97, np.maximum(w[2], 3.0), np.maximum(h[2], 3.0)
        if rotated:
            cols = [cx, cy, w, h, rs.uniform(-90, 90, (B, K)), score, cls]
        else:
            cols = [cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2, score, cls]
        table = np.stack(cols, -1).astype(F)
        if not full:
            table[2, 3, -2:] = (0.99, 1.5)                      # a class that is no integer
            table[2, 5, 0], table[2, 5, -2] = np.nan, 0.99     # geometry that is not a number
            table[2, 66, 1], table[2, 66, -2] = np.inf, 0.99
        return table
    return _frozen(('dets', rotated, full), make)


def kps(J):
    """[B, K, J, 2] float32: joints all over and up to three cells outside the map; in every row joint (row % J) is one of
    seven special values in turn: NaN x, infinite y, x = 0, x = MAP_W, y = 0, y = MAP_H (each exactly), both NaN."""
    def make():
        rs = np.random.RandomState(100 + J)
        table = np.stack([rs.uniform(-3, MAP_W + 3, (B, K, J)), rs.uniform(-3, MAP_H + 3, (B, K, J))], -1).astype(F)
        for b in range(B):
            for k in range(K):
                j, which = k % J, (k + b) % 7
                inside = (F(rs.uniform(1, MAP_W - 1)), F(rs.uniform(1, MAP_H - 1)))
                table[b, k, j] = [(np.nan, inside[1]), (inside[0], -np.inf), (0, inside[1]), (MAP_W, inside[1]),
                                  (inside[0], 0), (inside[0], MAP_H), (np.nan, np.nan)][which]
        return table
    return _frozen(('kps', J), make)


# ---------------------------------------------------------------------------------------------------------------------
# stage 2: a label table with joints, and the views
# ---------------------------------------------------------------------------------------------------------------------
COUNTS = (0, 1, K)
VIEWS = ('rot33', 'shift', 'ident')


def labels(rotated, J):
    """The dict cnuda_pseudo_labels_kps leaves, with COUNTS rows per image: boxes with centres all over the map and sides
    of 0.6 to 8 cells (the one row of image 1: 4 x 3 cells at the centre), joints up to three cells outside, visibility
    0, 1 (never kept by a view but the identity) and mostly 2; a few joints are not finite, with v = 2 among them."""
    def make():
        rs = np.random.RandomState(7 + 2 * J + rotated)
        cx, cy = rs.uniform(-1, MAP_W + 1, (B, K)), rs.uniform(-1, MAP_H + 1, (B, K))
        w, h = rs.uniform(0.6, 8, (B, K)), rs.uniform(0.6, 8, (B, K))
        cx[1, 0], cy[1, 0], w[1, 0], h[1, 0] = MAP_W / 2, MAP_H / 2, 4.0, 3.0
        if rotated:
            t = np.radians(rs.uniform(-90, 90, (B, K)))
            ox, oy = np.stack([-w, w, w, -w], -1) / 2, np.stack([-h, -h, h, h], -1) / 2
            geom = np.stack([cx[..., None] + ox * np.cos(t)[..., None] - oy * np.sin(t)[..., None],
                             cy[..., None] + ox * np.sin(t)[..., None] + oy * np.cos(t)[..., None]], -1)
        else:
            geom = np.stack([cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2], -1)
        classes = rs.randint(0, C, (B, K)).astype(np.int32)
        # whole cells and halves: a shift by whole cells lands joints on the map's edges exactly
        joints = np.stack([rs.randint(-6, 2 * MAP_W + 7, (B, K, J)), rs.randint(-6, 2 * MAP_H + 7, (B, K, J))], -1) / 2.0
        vis = rs.choice(np.int32([0, 1, 2, 2, 2, 2]), (B, K, J)).astype(np.int32)
        for b in range(B):
            for k in range(K):
                j, which = k % J, (k // J) % 5
                if which == 0:
                    joints[b, k, j], vis[b, k, j] = (np.nan, 3.0), 2
                elif which == 1:
                    joints[b, k, j], vis[b, k, j] = (5.0, np.inf), 2
                elif which == 2:
                    joints[b, k, j], vis[b, k, j] = (MAP_W - 3.0, 6.0), 2          # 'shift': x' = MAP_W exactly
                elif which == 3:
                    joints[b, k, j], vis[b, k, j] = (-3.0, 2.0), 2                  # 'shift': (0, 0) exactly
        for b, n in enumerate(COUNTS):
            geom[b, n:], classes[b, n:], joints[b, n:], vis[b, n:] = 0, 0, 0, 0
        return {'corners' if rotated else 'boxes': geom.astype(D), 'classes': classes, 'counts': np.int32(COUNTS),
                'kept': F(sum(COUNTS) / B), 'keypoints': joints.astype(D), 'visibility': vis,
                'joints': F(D(int((vis == 2).sum())) / D(B))}
    return _frozen(('labels', rotated, J), make)


def forward_maps(view):
    """[3, 6] float64 at map resolution.  'rot33': three similarities of the 4 x larger input (datasets.geometric_view);
    'shift': every image three cells to the right and two up -- whole cells, so that joints land on the map's edges
    exactly; 'ident': the identity on image 2 (its K rows), a similarity on the others."""
    def make():
        from datasets.geometric_view import GeometricViewParams, similarity_matrices
        p = GeometricViewParams.identity(B)
        for b, (angle, scale, shift) in enumerate([(33.0, 0.8, (0.13, -0.07)), (12.0, 1.0, (0.02, 0.0)),
                                                   (-33.0, 1.25, (-0.05, 0.1))]):
            p.forward[b], p.inverse[b] = similarity_matrices(4 * MAP_H, 4 * MAP_W, angle, scale, shift)
        six = p.forward_map(4)
        if view == 'shift':
            six = np.tile(D([1, 0, 3, 0, 1, -2]), (B, 1))
        elif view == 'ident':
            six[2] = (1, 0, 0, 0, 1, 0)
        return np.ascontiguousarray(six, dtype=D)
    return _frozen(('view', view), make)
