"""Seeded "trained-like" inputs of the box decode (decode.hip `decode_boxes_kernel`) at small shapes: head maps whose regression rows reach
every branch of the decode, and the per-class top-K lists fed to it.  Plain numpy; read by tests/test_decode_ref_cpu.py,
tests/test_gpu_decode_boxes.py and oracle/gen_golden.py (case `decode_structured`).

Seeded-noise head maps (N(0, 0.7) regression values, f_u = 721.5) leave most of the decode on a clamp: every keypoint depth
f_u h / (4 relu(dy) + 1e-3) is 100 m unless dy > ~2.6.  Here every pixel of a (B, 24, 40) map carries a row drawn as a trained model would
produce it: keypoint spans of several cells, depths of 2-90 m, uncertainties on both sides of 1 -- and, in stated shares, the values that sit
on each clamp.  `census` counts the branches from the float64 restatement alone; the CPU tests assert its shares.
"""
import numpy as np

from tests import decode_ref as D

H, W = 24, 40
NCLS = 3
H_NOMINAL = 1.67              # between the three class means of the height (1.5261, 1.7607, 1.7372)
SCORE_CLAMP = np.float32(1.0) - np.float32(1e-4)      # the heat map's upper clamp (layers/utils.py:39-43), as the device forms it

# Four images: a different pad, size and calibration each.  Images 0 and 2 are P2-like (b_x < 0), 1 and 3 P3-like (b_x > 0); the intrinsics
# are a KITTI camera's scaled to the 160 x 96 frame and are exact in float32.  pad = (frame - size) / 2, the dataset's centre pad.
IMAGES = (
    dict(size=(136, 80), pad=(12, 8), fu=180.375, fv=180.375, cu=76.25, cv=43.5, p03=11.25, p13=0.0546875),
    dict(size=(150, 90), pad=(5, 3), fu=176.5, fv=178.25, cu=80.125, cv=46.75, p03=-84.875, p13=0.6015625),
    dict(size=(124, 72), pad=(18, 12), fu=190.75, fv=189.5, cu=66.5, cv=40.25, p03=12.0, p13=-0.5),
    dict(size=(144, 86), pad=(8, 5), fu=172.25, fv=172.25, cu=72.0, cv=50.5, p03=-80.5, p13=0.25),
)


def image_P(i):
    """The 3 x 4 projection matrix of image i (what the reference's Calibration reads)."""
    m = IMAGES[i]
    return np.array([[m["fu"], 0, m["cu"], m["p03"]], [0, m["fv"], m["cv"], m["p13"]], [0, 0, 1, 0.0027]], dtype=np.float64)


def image_calib(i):
    """[f_u, f_v, c_u, c_v, b_x, b_y] in float32, derived as data/datasets/kitti_utils.py:213-218."""
    m = IMAGES[i]
    return np.array([m["fu"], m["fv"], m["cu"], m["cv"], m["p03"] / -m["fu"], m["p13"] / -m["fv"]], dtype=np.float32)


def regression_rows(rng, n, fu):
    """n rows of the 50 regression channels (key2channel order of runs/monoflex.yaml) for a camera of focal length fu."""
    r = np.zeros((n, D.R_TOTAL))
    # 2D extents, in cells: small, large (clips the box at a side), or negative (the relu branch)
    kind = rng.choice(3, size=(n, 4), p=(0.5, 0.3, 0.2))
    r[:, 0:4] = np.where(kind == 0, rng.uniform(0, 2.5, (n, 4)), np.where(kind == 1, rng.uniform(2.5, 14, (n, 4)), -rng.uniform(0, 2, (n, 4))))
    r[:, 1] *= 0.6
    r[:, 3] *= 0.6                                                    # the map is 24 cells high and 40 wide
    r[:, D.R_OFF3D:D.R_OFF3D + 2] = rng.normal(0, 0.5, (n, 2))
    r[:, D.R_DIM3D:D.R_DIM3D + 3] = rng.uniform(-1.5, 1.5, (n, 3))
    # keypoint y-spans: term t = f_u h / (4 dy) drawn around a base depth of 3-70 m; 12 % of the terms above the 100 m clamp (their pair's
    # mean may stay below it), 8 % with dy <= 0 (a quarter of those exactly 0): the relu and eps branch
    h = np.exp(r[:, D.R_DIM3D + 1]) * H_NOMINAL
    z = np.exp(rng.uniform(np.log(3.0), np.log(70.0), n))[:, None] * np.exp(rng.normal(0, 0.12, (n, 5)))
    what = rng.choice(3, size=(n, 5), p=(0.8, 0.12, 0.08))
    z = np.where(what == 1, rng.uniform(110, 180, (n, 5)), z)
    dy = fu * h[:, None] / (4 * z)
    neg = -rng.uniform(0, 2, (n, 5)) * (rng.uniform(size=(n, 5)) < 0.75)
    dy = np.where(what == 2, neg, dy)
    r[:, D.R_KPT:D.R_KPT + 20] = rng.normal(0, 2.0, (n, 20))         # x of every keypoint, y of the lower one of each pair
    ky = lambda k: D.R_KPT + 2 * k + 1
    for t, (top, bottom) in enumerate(((8, 9), (0, 4), (2, 6), (1, 5), (3, 7))):
        r[:, ky(top)] = r[:, ky(bottom)].astype(np.float32).astype(np.float64) + dy[:, t]
    # depth logit x: depth = exp(-x), log-uniform over 0.03-300 m (past both clamps), and +-100 (exp overflows float32 at -100)
    x = -rng.uniform(np.log(0.03), np.log(300.0), n)
    pick = rng.uniform(size=n)
    r[:, D.R_DEPTH] = np.where(pick < 0.08, 100.0, np.where(pick < 0.16, -100.0, x))
    # uncertainty logits in [-7, 3]: a level per row and a spread per estimate, so that sigma reaches 0.01 and 1 in every mode
    lvl = rng.uniform(-6.5, 2.5, n)[:, None] + rng.uniform(-0.5, 0.5, (n, 4))       # (no clipping: two estimates never share a value)
    r[:, D.R_DEPTH_UNC] = lvl[:, 0]
    r[:, D.R_KPT_UNC:D.R_KPT_UNC + 3] = lvl[:, 1:]
    # orientation: every bin wins in a quarter of the rows; the angle of bin 3 (centre -pi/2) leans negative so that alpha wraps upward too
    win = rng.integers(0, 4, n)
    a = rng.normal(0, 1, (n, 4))
    gap = np.where(np.arange(4)[None, :] == win[:, None], rng.uniform(0.6, 3, (n, 4)), rng.uniform(-3, 0.4, (n, 4)))
    r[:, D.R_ORI_CLS:D.R_ORI_CLS + 8:2] = a
    r[:, D.R_ORI_CLS + 1:D.R_ORI_CLS + 8:2] = a + gap
    theta = rng.uniform(-np.pi, np.pi, (n, 4))
    theta[:, 3] = rng.uniform(-np.pi, 0, n)
    rad = rng.uniform(0.3, 2, (n, 4))
    r[:, D.R_ORI_OFF:D.R_ORI_OFF + 8:2] = rad * np.sin(theta)
    r[:, D.R_ORI_OFF + 1:D.R_ORI_OFF + 8:2] = rad * np.cos(theta)
    return r.astype(np.float32)


def structured_maps(seed, images=(0, 1, 2), ld=64, reg_off=8):
    """-> dict(hmap (B,H,W,ld) float32, calib (B,6) float32, pad (B,2) int32, sizes (B,2) int32, img_size (2,) int32 = image 0's).
    Every pixel holds a structured row at [reg_off, reg_off + 50); the other channels hold noise a wrong offset would read."""
    assert reg_off + D.R_TOTAL <= ld
    rng = np.random.default_rng(seed)
    B = len(images)
    hmap = rng.normal(0, 3, (B, H, W, ld)).astype(np.float32)
    for b, i in enumerate(images):
        hmap[b, :, :, reg_off:reg_off + D.R_TOTAL] = regression_rows(rng, H * W, IMAGES[i]["fu"]).reshape(H, W, D.R_TOTAL)
    sizes = np.array([IMAGES[i]["size"] for i in images], dtype=np.int32)
    return dict(hmap=hmap, calib=np.stack([image_calib(i) for i in images]), pad=np.array([IMAGES[i]["pad"] for i in images], dtype=np.int32),
                sizes=sizes, img_size=sizes[0].copy(), images=tuple(images), ld=ld, reg_off=reg_off)


LIST_KINDS = ("distinct", "ties", "shared_pixel", "threshold")
THRESHOLD = 0.2


def _distinct_scores(rng, n, lo, hi):
    """n distinct float32 scores in (lo, hi)."""
    s = (lo + (hi - lo) * (rng.permutation(n) + 0.5 + rng.uniform(-0.4, 0.4, n)) / n).astype(np.float32)
    assert np.unique(s).size == n
    return s


def score_lists(seed, B, K, kind="distinct", lo=0.02, hi=0.98):
    """-> scores (B, 3, K) float32, each class's list in descending order as stage 1 leaves it, and index (B, 3, K) int32, K distinct pixels
    per class.
      distinct      no two scores of an image equal
      ties          the first max(1, K // 4) scores of EVERY class are exactly the clamp value 0.9999, and one lower value is shared by all
                    three classes: stage 2 must order equals by their position in the (3 K) list
      shared_pixel  as `distinct`, with pixels that appear in two (one of them in all three) classes
      threshold     scores exactly at the 0.2 threshold, one ulp below and one ulp above, in different classes"""
    assert kind in LIST_KINDS and 1 <= K <= H * W
    rng = np.random.default_rng(seed)
    scores = _distinct_scores(rng, B * NCLS * K, lo, hi).reshape(B, NCLS, K)
    index = np.stack([np.stack([rng.choice(H * W, K, replace=False) for _ in range(NCLS)]) for _ in range(B)]).astype(np.int32)
    thr = np.float32(THRESHOLD)
    if kind == "ties":
        scores[:, :, :max(1, K // 4)] = SCORE_CLAMP
        if K >= 4:
            scores[:, :, K // 4] = np.float32(0.75)
    elif kind == "shared_pixel":
        index[:, 1, 0] = index[:, 0, 0]
        if K > 2:
            index[:, 2, K // 2] = index[:, 0, K // 2]
            index[:, 1, K // 2] = index[:, 0, K // 2]
            index[:, 2, K - 1] = index[:, 1, K - 2]
        for b in range(B):                                            # (the pixels of one class stay distinct)
            for c in range(NCLS):
                if np.unique(index[b, c]).size != K:
                    return score_lists(seed + 7919, B, K, kind, lo, hi)
    elif kind == "threshold":
        vals = (thr, np.nextafter(thr, np.float32(0)), np.nextafter(thr, np.float32(1)))
        scores = -np.sort(-scores, axis=2)
        low = (0.02 + (scores[:, :, K // 4:].astype(np.float64) - 0.02) * 0.17).astype(np.float32)   # all but a quarter of each list below 0.19:
        assert np.unique(low).size == low.size                                                        # the planted values reach the merged top K
        scores[:, :, K // 4:] = low
        for c in range(NCLS):
            scores[:, c, K - 1] = vals[c]
            if K >= 2:
                scores[:, c, K - 2] = vals[(c + 1) % 3]               # (so every planted value appears twice, in two classes)
    scores = -np.sort(-scores, axis=2)
    return np.ascontiguousarray(scores), np.ascontiguousarray(index)


def peak_lists(seed, B, K, ranges=None):
    """Lists whose pixels can be isolated peaks of a class heat map: each class takes K pixels of a 2-cell lattice (no two 8-neighbours), the
    lattice's parity changing from image to image so that the last row and column are reached; all scores of an image distinct.
    `ranges`: per image (lo, hi) of the scores."""
    rng = np.random.default_rng(seed)
    scores, index = np.zeros((B, NCLS, K), dtype=np.float32), np.zeros((B, NCLS, K), dtype=np.int32)
    for b in range(B):
        oy, ox = (b // 2) % 2, b % 2
        lattice = np.array([(y * W + x) for y in range(oy, H, 2) for x in range(ox, W, 2)])
        assert K <= lattice.size
        lo, hi = (0.02, 0.98) if ranges is None else ranges[b]
        scores[b] = -np.sort(-_distinct_scores(rng, NCLS * K, lo, hi).reshape(NCLS, K), axis=1)
        for c in range(NCLS):
            index[b, c] = rng.choice(lattice, K, replace=False)
    return scores, index


BACKGROUND_LOGIT = -12.0       # sigmoid = 6e-6: the heat map's lower clamp 1e-4, below every peak


def peak_heat(scores, index, b):
    """Class heat map (3, H, W) float32 of image b after sigmoid/clamp: the lists' scores at their pixels, the lower clamp elsewhere."""
    heat = np.full((NCLS, H * W), 1e-4, dtype=np.float32)
    for c in range(NCLS):
        heat[c, index[b, c]] = scores[b, c]
    return heat.reshape(NCLS, H, W)


def peak_logits(scores, index):
    """Class logits (B, H, W, 3) float32 with isolated peaks: logit(score) at the lists' pixels, BACKGROUND_LOGIT elsewhere."""
    B = scores.shape[0]
    lg = np.full((B, H * W, NCLS), BACKGROUND_LOGIT, dtype=np.float32)
    s = scores.astype(np.float64)
    for b in range(B):
        for c in range(NCLS):
            lg[b, index[b, c], c] = np.log(s[b, c] / (1 - s[b, c])).astype(np.float32)
    return lg.reshape(B, H, W, NCLS)


# ---- census ------------------------------------------------------------------------------------------------------------------------------
def census(ref, mode):
    """Share of the rows of a decode_ref result that take each branch -> {name: (share, least share taken, least share missed)}."""
    n = ref["det"].shape[0] * ref["det"].shape[1]
    t = ref["kpt_terms"].reshape(n, 5)
    dy = ref["kpt_dy"].reshape(n, 5)
    raw = ref["box_raw"].reshape(n, 4)
    wmax = np.repeat(ref["box_max"][:, 0], ref["det"].shape[1])
    hmax = np.repeat(ref["box_max"][:, 1], ref["det"].shape[1])
    flat = lambda k: ref[k].reshape(n)
    dmax = 100.0
    in_range = ((t >= 2) & (t <= 90)).all(axis=1)
    clip = dict(left=(raw[:, 0] < 0) | (raw[:, 2] < 0), top=(raw[:, 1] < 0) | (raw[:, 3] < 0),
                right=(raw[:, 0] > wmax) | (raw[:, 2] > wmax), bottom=(raw[:, 1] > hmax) | (raw[:, 3] > hmax))
    c = {
        "all five keypoint terms in 2-90 m": (in_range, 0.10, 0.10),
        "d1 below the 100 m clamp": (flat("d1_raw") < dmax, 0.10, 0.10),
        "d2 below the 100 m clamp": (flat("d2_raw") < dmax, 0.10, 0.10),
        "d3 below the 100 m clamp": (flat("d3_raw") < dmax, 0.10, 0.10),
        "d2: one term above 100 m, the other below": ((t[:, 1] > dmax) != (t[:, 2] > dmax), 0.10, 0.10),
        "d3: one term above 100 m, the other below": ((t[:, 3] > dmax) != (t[:, 4] > dmax), 0.10, 0.10),
        "a keypoint span dy <= 0 (relu, eps)": ((dy <= 0).any(axis=1), 0.10, 0.10),
        "direct depth at the 0.1 m clamp": (flat("d_direct_raw") < 0.1, 0.10, 0.10),
        "direct depth at the 100 m clamp": (flat("d_direct_raw") > dmax, 0.10, 0.10),
        "sigma at the 0.01 clamp": (flat("sigma") < 0.01, 0.10, 0.10),
        "sigma at the clamp of 1": (flat("sigma") > 1, 0.10, 0.10),
        "alpha wraps down (> pi)": (flat("alpha_raw") > np.pi, 0.05, 0.05),
        "alpha wraps up (< -pi)": (flat("alpha_raw") < -np.pi, 0.05, 0.05),
        "ry wraps down (> pi)": (flat("ry_raw") > np.pi, 0.05, 0.05),
        "ry wraps up (< -pi)": (flat("ry_raw") < -np.pi, 0.05, 0.05),
        "2D box clear of every side": (~(clip["left"] | clip["top"] | clip["right"] | clip["bottom"]), 0.05, 0.05),
    }
    for side, m in clip.items():
        c["2D box clipped at the %s side" % side] = (m, 0.05, 0.05)
    for i in range(4):
        c["orientation bin %d wins" % i] = (flat("best_bin") == i, 0.10, 0.10)
    if mode == "hard":
        for i in range(4):
            c["hard: estimate %d has the largest weight" % i] = (flat("hard_choice") == i, 0.10, 0.10)
    return {k: (float(np.mean(m)), lo, miss) for k, (m, lo, miss) in c.items()}


def format_census(c):
    return "\n".join("  %-48s %5.1f %%" % (k, 100 * v[0]) for k, v in c.items())


# ---- the cases the device tests run (tests/test_gpu_decode_boxes.py); the CPU census holds for each of them --------------------------------
CASES = {
    "b3_k50": dict(seed=11, images=(0, 1, 2), K=50, ld=64, reg_off=8),
    "b3_permuted": dict(seed=12, images=(2, 0, 1), K=50, ld=64, reg_off=8),       # image 0 is now the smallest frame: its size clamps all three
    "b1_k100": dict(seed=13, images=(3,), K=100, ld=64, reg_off=8),
    "k1": dict(seed=14, images=(0, 1, 2), K=1, ld=64, reg_off=8),
    "k7": dict(seed=15, images=(0, 1, 2), K=7, ld=64, reg_off=8),
    "k100": dict(seed=16, images=(0, 1, 2), K=100, ld=64, reg_off=8),
    "k256": dict(seed=17, images=(0, 1, 2), K=256, ld=64, reg_off=8),
    "ld50": dict(seed=18, images=(0, 1, 2), K=50, ld=50, reg_off=0),
    "ld72": dict(seed=19, images=(0, 1, 2), K=50, ld=72, reg_off=13),
}
CENSUS_MIN_ROWS = 100          # the shares are asserted for every case with at least this many rows (k1 and k7 have 3 and 21)


def case_inputs(name, kind="distinct"):
    """The maps and lists of one case -> dict(hmap, reg_off, scores, index, calib, pad, img_size, sizes, threshold)."""
    c = CASES[name]
    m = structured_maps(c["seed"], c["images"], c["ld"], c["reg_off"])
    scores, index = score_lists(c["seed"] + 1000, len(c["images"]), c["K"], kind)
    return dict(m, scores=scores, index=index, threshold=THRESHOLD)


def run_ref(d, mode, **kw):
    return D.decode_boxes(d["hmap"], d["reg_off"], d["scores"], d["index"], d["calib"], d["pad"], d["img_size"], d["threshold"], mode,
                          img_sizes=d["sizes"], **kw)


def lattice_lists(seed, parity, H_=H, W_=W):
    """One image's lists (1, 3, 240) covering EVERY pixel of the 2-cell lattice of the given parity (0..3) once: 80 isolated peaks per
    class, distinct scores; the rest of each class's list is padding at the heat map's lower clamp that never reaches the merged top 240.
    Four parities decode every pixel of a map."""
    rng = np.random.default_rng(seed)
    oy, ox = parity // 2, parity % 2
    lattice = rng.permutation(np.array([(y * W_ + x) for y in range(oy, H_, 2) for x in range(ox, W_, 2)]))
    n = lattice.size // NCLS
    scores = -np.sort(-_distinct_scores(rng, NCLS * n, 0.02, 0.98).reshape(1, NCLS, n), axis=2)
    return scores, lattice[:NCLS * n].reshape(1, NCLS, n).astype(np.int32)
