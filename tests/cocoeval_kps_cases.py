"""Seeded inputs of the keypoint-evaluation tests (tests/test_host_cocoeval_kps.py, tests/test_gpu_cocoeval_kps.py):
`add_batch` keyword dictionaries, the smallest that reach every path.  Batch one: 3 images of 384 x 384, 3 classes, 30
predictions and up to 8 ground truths each; areas on both sides of 32^2 and 96^2; COCO's v in {0, 1, 2}, ground
truths without a labelled joint among them; predictions jittered around the ground truths by 0.3 to 5 times
sigma_j * sqrt(area), so the similarity spreads over (0, 1).  Batch two: 25 predictions x 70 ground truths of one class
(the cut to 20; a lane of the matcher owns two ground truths), 20 x 120 (2400 pairs: more than one pass of the
pair kernel's 8 x 256 threads), an image without ground truth and one without a prediction above the threshold."""
import numpy as np

SHAPE = (3, 384, 384)
SIGMAS3 = (0.05, 0.1, 0.07)
PERSON = (0.026, 0.025, 0.025, 0.035, 0.035, 0.079, 0.079, 0.072, 0.072, 0.062, 0.062, 0.107, 0.107, 0.087, 0.087, 0.089,
          0.089)
SPREAD = (0.3, 1.0, 1.5, 2.0, 3.0, 5.0)


def sigmas_of(J):
    return np.array(SIGMAS3 if J == 3 else PERSON, dtype=np.float64)


def _image(rng, J, K, G, classes, n_pred, first_unlabelled=None):
    """-> pred boxes [K, 4], classes [K], scores [K], kps [K, J, 2]; gt boxes [G, 4], classes [G], areas [G], kps [G, J, 3].
    The first `n_pred` predictions score above the threshold."""
    sig = sigmas_of(J)
    side = rng.choice([20.0, 28.0, 40.0, 70.0, 110.0, 150.0], G) * rng.uniform(0.8, 1.2, G)
    w, h = side * rng.uniform(0.7, 1.3, G), side
    x0, y0 = rng.uniform(0, 384 - w), rng.uniform(0, 384 - h)
    gt_boxes = np.stack([x0, y0, x0 + w, y0 + h], 1).astype(np.float32)
    areas = (w * h * rng.uniform(0.5, 0.9, G)).astype(np.float32)              # segment areas: below the box's
    true = np.stack([x0[:, None] + rng.uniform(0, 1, (G, J)) * w[:, None],
                     y0[:, None] + rng.uniform(0, 1, (G, J)) * h[:, None]], 2)
    vis = rng.choice([0, 1, 2], (G, J), p=[0.25, 0.25, 0.5])
    unlabelled = np.arange(G) % 4 == 3 if first_unlabelled is None else np.arange(G) < first_unlabelled
    vis[unlabelled] = 0
    vis[~unlabelled, 0] = 2                                                   # the others keep at least one joint
    gt_kps = np.concatenate([np.where(vis[:, :, None] > 0, true, 0.0), vis[:, :, None]], 2).astype(np.float32)
    gc = rng.randint(0, classes, G)
    if G:
        src = rng.randint(0, G, K)
        scale = rng.choice(SPREAD, K)[:, None, None] * sig[None, :, None] * np.sqrt(areas[src].astype(np.float64))[:, None, None]
        pred_kps = true[src] + rng.normal(0, 1, (K, J, 2)) * scale
        # every fifth prediction of an unlabelled ground truth lands partly outside its doubled box
        far = unlabelled[src] & (np.arange(K) % 5 == 0)
        pred_kps[far, 0, 0] = (x0 + 2 * w)[src][far] + scale[far, 0, 0] * rng.uniform(0.5, 1.5, int(far.sum()))
        pred_boxes = gt_boxes[src] + rng.normal(0, 2, (K, 4))
        pc = np.where(rng.uniform(size=K) < 0.85, gc[src], rng.randint(0, classes, K))
    else:
        pred_kps = rng.uniform(0, 384, (K, J, 2))
        pred_boxes = np.stack([pred_kps[:, :, 0].min(1), pred_kps[:, :, 1].min(1), pred_kps[:, :, 0].max(1),
                               pred_kps[:, :, 1].max(1)], 1)
        pc = rng.randint(0, classes, K)
    scores = np.sort(rng.uniform(0.11, 1.0, K).astype(np.float32))[::-1].copy()
    scores[3:n_pred:7] = np.float32(0.5)                                      # equal scores: the stable sorts decide
    scores[n_pred:] = rng.uniform(0.0, 0.09, K - n_pred).astype(np.float32)
    order = rng.permutation(K)
    return (pred_boxes[order].astype(np.float32), pc[order].astype(np.int32), scores[order],
            pred_kps[order].astype(np.float32), gt_boxes, gc.astype(np.int32), areas, gt_kps)


def _batch(images, first_id):
    return {'pred_boxes': np.stack([im[0] for im in images]), 'pred_classes': np.stack([im[1] for im in images]),
            'pred_scores': np.stack([im[2] for im in images]), 'pred_kps': np.stack([im[3] for im in images]),
            'gt_boxes': [im[4] for im in images], 'gt_classes': [im[5] for im in images],
            'gt_areas': [im[6] for im in images], 'gt_kps': [im[7] for im in images],
            'gt_ids': [np.int64(first_id + i) for i in range(len(images))], 'image_shape': SHAPE}


def case(J, seed=None):
    """-> [add_batch kwargs, add_batch kwargs] for J = 3 or 17"""
    rng = np.random.RandomState({3: 11, 17: 12}[J] if seed is None else seed)
    one = _batch([_image(rng, J, 30, G, 3, 30) for G in (8, 6, 8)], 900 + 100 * J)
    two = _batch([_image(rng, J, 30, 70, 1, 25, first_unlabelled=6),        # 25 x 70 of one class: cut to 20
                  _image(rng, J, 30, 120, 1, 20, first_unlabelled=9),       # 20 x 120 = 2400 pairs
                  _image(rng, J, 30, 0, 3, 12),                             # no ground truth
                  _image(rng, J, 30, 5, 3, 0)],                             # no prediction above the threshold
                 950 + 100 * J)
    return [one, two]


def two_columns(batch):
    """the batch with `gt_kps` as [n, J, 2]"""
    return dict(batch, gt_kps=[k[:, :, :2] for k in batch['gt_kps']])


def all_visible(batch):
    """the batch with every v = 2"""
    out = []
    for k in batch['gt_kps']:
        k = k.copy()
        k[:, :, 2] = 2
        out.append(k)
    return dict(batch, gt_kps=out)
