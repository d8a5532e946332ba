"""Plain fp64 numpy references of the detection tail (csrc/anchor_tail.hip; include/imvoxel.h states the operations), written from the
definitions and not from the kernels, with the case lists, the drivers and the checkers shared by tests/test_host_tail_fp64.py (the CPU
restatement oracle/cpu_abi, no device) and tests/test_gpu_tail_fp64.py (the HIP library).

Discrete outputs (indices, labels, counts, order) must be IDENTICAL to the reference's.  No case is excused after the fact: the inputs
are built so that the reference's own decisions are robust, and the drivers assert it -- unequal scores that decide something differ by
at least SCORE_MARGIN relative, every IoU that decides something is at least IOU_MARGIN from the threshold, no fixed-up yaw is within
YAW_MARGIN of a period boundary.

Continuous outputs are bounded by counting roundings, in units of U = 2^-24 times the magnitude the cancellation runs over (as
ref_ops.dcn_bound does).  The HIP math documentation is not available to this suite, so every expf / sinf / cosf / sqrtf / atan2f call
is counted at 2 ulp = 4 U.  The rotated overlap has no useful a-priori count: its bound per configuration class is the measured error of
the C oracle (OVERLAP_MEASURED below), and the device and the CPU restatement must stay within OVERLAP_SLACK = 4 times that."""
import ctypes as C

import numpy as np

U = 2.0 ** -24                   # one fp32 rounding, relative
ULP2 = 4.0                       # a libm call (expf, sinf, cosf, sqrtf) in units of U: 2 ulp
SECOND = 1.0 + 2.0 ** -10        # second-order terms of the products of (1 + k U) factors
TINY = 2.0 ** -126               # below the normal range a rounding is absolute
PI32 = float(np.float32(np.pi))  # the kernel's IVX_PI_F
SCORE_MARGIN = 1e-4
IOU_MARGIN = 1e-3
YAW_MARGIN = 1e-3

K_SIGMOID = 6                    # expf(-x): 4 | 1 + e: 1 (the error of e enters with e / (1 + e) < 1, counted in the 4) | 1 / .: 1
K_XY = 7                         # diag = sqrtf(l*l + w*w): (1 + 1 weighted + 1) / 2 + 4 = 5 | xt * diag: 1 | + xa: 1      on |xt diag| + |xa|
K_Z = 9                          # za + ha/2: 1 | zt * ha: 1 | + : 1 | hg = expf * ha: 5 (on hg / 2) | zg - hg/2: 1       on |za| + |ha/2| + |zt ha| + |hg/2|
K_SIZE = 5                       # expf: 4 | * anchor size: 1                                                              on the size itself
K_ROT = 1                        # rt + ra: 1                                                                              on |rt| + |ra|
K_YAW = 6                        # rg: 1 | - dir_offset: 1 | t * pi: 1 | val - .: 1 | + dir_offset: 1 | + pi * dir: 1   (val / pi + limit only feeds the floor)
K_FCOS_SCORE = 13                # two sigmoids: 6 + 6 | their product: 1 | * valid (0 or 1): exact
K_POINT = 2                      # i * vs: 1 | + new_origin: 1                                                             on |i vs| + |origin|


# ------------------------------------------------------------------------------------------------------------------ geometry
def _corners(b):
    """[m, 5] (x1, y1, x2, y2, angle) -> [m, 4, 2] corners, rotated about the centre with x' = dx cos a + dy sin a, y' = -dx sin a + dy cos a"""
    b = np.asarray(b, np.float64).reshape(-1, 5)
    cx, cy = (b[:, 0] + b[:, 2]) / 2, (b[:, 1] + b[:, 3]) / 2
    hx, hy = (b[:, 2] - b[:, 0]) / 2, (b[:, 3] - b[:, 1]) / 2
    dx = np.stack([-hx, hx, hx, -hx], 1)
    dy = np.stack([-hy, -hy, hy, hy], 1)
    c, s = np.cos(b[:, 4])[:, None], np.sin(b[:, 4])[:, None]
    return np.stack([cx[:, None] + dx * c + dy * s, cy[:, None] - dx * s + dy * c], 2)


def _shoelace(P, cnt):
    """signed area of the polygons P [m, V, 2] with cnt [m] vertices each"""
    m, V, _ = P.shape
    rows = np.arange(m)
    area = np.zeros(m)
    for i in range(V):
        act = i < cnt
        nxt = P[rows, (i + 1) % np.maximum(cnt, 1)]
        area += np.where(act, P[:, i, 0] * nxt[:, 1] - nxt[:, 0] * P[:, i, 1], 0.0)
    return area / 2


def _clip_pairs(A, B):
    """area of the intersection of the convex quadrilaterals A [m, 4, 2] and B [m, 4, 2]: A clipped by the four half planes of B"""
    m = A.shape[0]
    rows = np.arange(m)
    flip = _shoelace(B, np.full(m, 4)) < 0                      # make B counter-clockwise: the inside is on the left of every edge
    B = np.where(flip[:, None, None], B[:, ::-1], B)
    P, cnt = np.zeros((m, 9, 2)), np.full(m, 4)
    P[:, :4] = A - B[:, :1]                                     # work relative to a corner of B: no cancellation against a far origin
    Bl = B - B[:, :1]
    for e in range(4):
        e0, e1 = Bl[:, e], Bl[:, (e + 1) % 4]
        ex, ey = e1[:, 0] - e0[:, 0], e1[:, 1] - e0[:, 1]

        def side(q):
            return ex * (q[:, 1] - e0[:, 1]) - ey * (q[:, 0] - e0[:, 0])
        out, oc = np.zeros_like(P), np.zeros(m, np.int64)
        for i in range(9):
            act = i < cnt
            if not act.any():
                break
            cur, prv = P[:, i], P[rows, (i - 1) % np.maximum(cnt, 1)]
            sc, sp = side(cur), side(prv)
            cin, pin = sc >= 0, sp >= 0
            cross = act & (cin != pin)
            idx = np.nonzero(cross)[0]
            t = sp[idx] / (sp[idx] - sc[idx])
            out[idx, oc[idx]] = prv[idx] + t[:, None] * (cur[idx] - prv[idx])
            oc[idx] += 1
            idx = np.nonzero(act & cin)[0]
            out[idx, oc[idx]] = cur[idx]
            oc[idx] += 1
        P, cnt = out, oc
    return np.abs(_shoelace(P, cnt))


def overlap_matrix(a, b):
    """[na, 5] x [nb, 5] -> [na, nb] fp64 intersection areas.  Pairs whose circumscribed circles are apart are 0 without clipping."""
    a, b = np.asarray(a, np.float64).reshape(-1, 5), np.asarray(b, np.float64).reshape(-1, 5)
    out = np.zeros((a.shape[0], b.shape[0]))
    if out.size == 0:
        return out
    ca, cb = np.stack([a[:, 0] + a[:, 2], a[:, 1] + a[:, 3]], 1) / 2, np.stack([b[:, 0] + b[:, 2], b[:, 1] + b[:, 3]], 1) / 2
    ra, rb = np.hypot(a[:, 2] - a[:, 0], a[:, 3] - a[:, 1]) / 2, np.hypot(b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]) / 2
    dist = np.hypot(ca[:, None, 0] - cb[None, :, 0], ca[:, None, 1] - cb[None, :, 1])
    i, j = np.nonzero(dist <= (ra[:, None] + rb[None, :]) * (1 + 1e-9))
    if i.size:
        out[i, j] = _clip_pairs(_corners(a)[i], _corners(b)[j])
    return out


def rect_overlap(a, b):
    """area of the intersection of two rotated rectangles (x1, y1, x2, y2, angle)"""
    return float(overlap_matrix(np.asarray(a).reshape(1, 5), np.asarray(b).reshape(1, 5))[0, 0])


def areas(b):
    b = np.asarray(b, np.float64).reshape(-1, 5)
    return (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])


def iou_bev_matrix(a, b):
    so = overlap_matrix(a, b)
    return so / np.maximum(areas(a)[:, None] + areas(b)[None, :] - so, 1e-8)


def iou_bev(a, b):
    return float(iou_bev_matrix(np.asarray(a).reshape(1, 5), np.asarray(b).reshape(1, 5))[0, 0])


def iou_axis_matrix(a, b):
    """the angle is ignored: nms_normal_gpu"""
    a, b = np.asarray(a, np.float64).reshape(-1, 5), np.asarray(b, np.float64).reshape(-1, 5)
    w = np.maximum(np.minimum(a[:, None, 2], b[None, :, 2]) - np.maximum(a[:, None, 0], b[None, :, 0]), 0)
    h = np.maximum(np.minimum(a[:, None, 3], b[None, :, 3]) - np.maximum(a[:, None, 1], b[None, :, 1]), 0)
    so = w * h
    return so / np.maximum(areas(a)[:, None] + areas(b)[None, :] - so, 1e-8)


def iou_axis(a, b):
    return float(iou_axis_matrix(np.asarray(a).reshape(1, 5), np.asarray(b).reshape(1, 5))[0, 0])


def greedy_nms(boxes_sorted, thr, rotated):
    """boxes in descending score.  Returns (kept indices, decision margin): the smallest |IoU - thr| over the pairs whose IoU decided
    something -- a kept box against a later box that nothing had removed yet."""
    b = np.asarray(boxes_sorted, np.float64).reshape(-1, 5)
    n = b.shape[0]
    thr = float(np.float32(thr))
    full = iou_bev_matrix(b, b) if rotated and n else None
    removed = np.zeros(n, bool)
    keep, margin = [], np.inf
    for i in range(n):
        if removed[i]:
            continue
        keep.append(i)
        if i + 1 == n:
            break
        row = full[i, i + 1:] if rotated else iou_axis_matrix(b[i:i + 1], b[i + 1:])[0]
        alive = ~removed[i + 1:]
        if alive.any():
            margin = min(margin, float(np.abs(row[alive] - thr).min()))
        removed[i + 1:] |= row > thr
    return np.array(keep, np.int64), margin


def topk(scores, k):
    """descending, ties to the lower index.  Returns (indices, margin): the smallest relative gap between unequal neighbours of the sorted
    list among the first k and across the cut (k-1 | k)."""
    s = np.asarray(scores, np.float64)
    n = s.shape[0]
    k = min(k, n)
    order = np.lexsort((np.arange(n), -s))
    top = s[order[:min(k + 1, n)]]
    gap = top[:-1] - top[1:]
    ne = gap > 0
    margin = float((gap[ne] / top[:-1][ne]).min()) if ne.any() else np.inf
    return order[:k], margin


def sigmoid(x):
    return 1.0 / (1.0 + np.exp(-np.asarray(x, np.float64)))


# ------------------------------------------------------------------------------------------------------------------ anchor head
def anchor_tail(head_out, anchors, d):
    """Anchor3DHead.get_bboxes_single for one sample.  head_out [H, W, CH] in (y, x) order whatever the memory layout (the driver undoes
    hw_transposed), anchors [H*W*A, 7], d a dict of the descriptor's fields.  Returns a dict: cand_idx, cand_boxes, cand_scores [k], their
    bounds, keep (positions among the candidates), out_boxes / out_scores [count], bounds, dir, margins."""
    H, W, A = d['H'], d['W'], d['num_anchors']
    n = H * W * A
    ho = np.asarray(head_out, np.float64).reshape(H * W, -1)
    an = np.asarray(anchors, np.float64).reshape(n, 7)
    cls = ho[:, d['cls_off']:d['cls_off'] + A].reshape(n)
    reg = ho[:, d['reg_off']:d['reg_off'] + 7 * A].reshape(n, 7)
    dr = ho[:, d['dir_off']:d['dir_off'] + 2 * A].reshape(n, 2)
    score = sigmoid(cls)
    k = d['nms_pre'] if 0 < d['nms_pre'] < n else n
    idx, smargin = topk(score, k)
    thr = float(np.float32(d['score_thr']))
    sc = score[idx]
    n1 = int((sc > thr).sum())
    # a score at rounding distance of score_thr would make n1 undefined: exactly equal is allowed only where fp32 gives it exactly too (logit 0)
    near = np.abs(sc - thr) / max(thr, 1e-30)
    tmargin = float(near[near > 0].min()) if (near > 0).any() else np.inf
    t, a = reg[idx], an[idx]
    xa, ya, za, wa, la, ha, ra = a.T
    diag = np.sqrt(la * la + wa * wa)
    za_c = za + ha / 2
    hg = np.exp(t[:, 5]) * ha
    boxes = np.stack([t[:, 0] * diag + xa, t[:, 1] * diag + ya, t[:, 2] * ha + za_c - hg / 2, np.exp(t[:, 3]) * wa, np.exp(t[:, 4]) * la, hg,
                      t[:, 6] + ra], 1)
    mag = np.stack([np.abs(t[:, 0] * diag) + np.abs(xa), np.abs(t[:, 1] * diag) + np.abs(ya),
                    np.abs(za) + np.abs(ha / 2) + np.abs(t[:, 2] * ha) + np.abs(hg / 2), boxes[:, 3], boxes[:, 4], boxes[:, 5],
                    np.abs(t[:, 6]) + np.abs(ra)], 1)
    Kb = np.array([K_XY, K_XY, K_Z, K_SIZE, K_SIZE, K_SIZE, K_ROT], np.float64)
    bbound = Kb * U * SECOND * mag + TINY
    bev = np.stack([boxes[:, 0] - boxes[:, 3] / 2, boxes[:, 1] - boxes[:, 4] / 2, boxes[:, 0] + boxes[:, 3] / 2, boxes[:, 1] + boxes[:, 4] / 2,
                    boxes[:, 6]], 1)
    direction = (dr[idx, 1] > dr[idx, 0]).astype(np.int64)               # a tie gives 0
    keep, imargin = greedy_nms(bev[:n1], d['nms_thr'], bool(d['use_rotate_nms']))
    keep = keep[:d['max_num']]
    off, lim = float(np.float32(d['dir_offset'])), float(np.float32(d['dir_limit_offset']))
    val = boxes[keep, 6] - off
    q = val / PI32 + lim
    tt = np.floor(q)
    ymargin = float(np.minimum(q - tt, tt + 1 - q).min()) * PI32 if keep.size else np.inf
    yaw = val - tt * PI32 + off + PI32 * direction[keep]
    ob = boxes[keep].copy()
    ob[:, 6] = yaw
    obound = bbound[keep].copy()
    obound[:, 6] = K_YAW * U * SECOND * (np.abs(boxes[keep, 6]) + abs(off) + np.abs(tt * PI32) + PI32) + TINY
    return dict(k=k, n1=n1, cand_idx=idx, cand_boxes=boxes, cand_bound=bbound, cand_scores=sc, score_bound=K_SIGMOID * U * SECOND * sc + TINY,
                bev=bev, dir=direction, keep=keep, out_boxes=ob, out_bound=obound, out_scores=sc[keep],
                score_margin=smargin, thr_margin=tmargin, iou_margin=imargin, yaw_margin=ymargin)


# ------------------------------------------------------------------------------------------------------------------ FCOS level
def pooled_valid(valid0, level):
    """valid0 [X, Y, Z] bool -> the level's mask: level 0 itself; level l > 0 from the eight level-0 voxels (i << l) + 2^(l-1) - 1 + {0, 1}
    per axis, valid when at least 5 of them are set (the mean of 8 samples rounded half to even: 4 of 8 is 0)."""
    v = np.asarray(valid0).astype(np.int64)
    if level == 0:
        return v > 0
    h = (1 << (level - 1)) - 1
    st = 1 << level
    cnt = 0
    for a in (0, 1):
        for e in (0, 1):
            for f in (0, 1):
                cnt = cnt + v[h + a::st, h + e::st, h + f::st][:v.shape[0] >> level, :v.shape[1] >> level, :v.shape[2] >> level]
    return cnt >= 5


def fcos_level_candidates(head_out, valid0, vs, new_origin, scale, n_classes, R, level, nms_pre):
    """One sample.  head_out [nx, ny, nz, CH] = [centerness | R regression | classes | padding], vs / new_origin [3].
    Returns dict(idx, boxes [k, R], box_bound, scores [k, ncls], score_bound, margin)."""
    nx, ny, nz, CH = head_out.shape
    n = nx * ny * nz
    ho = np.asarray(head_out, np.float64).reshape(n, CH)
    vf = pooled_valid(valid0, level).reshape(n).astype(np.float64)
    scores = sigmoid(ho[:, 1 + R:1 + R + n_classes]) * sigmoid(ho[:, :1]) * vf[:, None]
    k = nms_pre if 0 < nms_pre < n else n
    idx, margin = topk(scores.max(1), k)
    ix, iy, iz = np.unravel_index(idx, (nx, ny, nz))
    vs, no = np.asarray(vs, np.float64), np.asarray(new_origin, np.float64)
    ijk = np.stack([ix, iy, iz], 1).astype(np.float64)
    pt = ijk * vs + no
    ept = K_POINT * U * (np.abs(ijk * vs) + np.abs(no))                                    # K_POINT, see above
    arg = ho[idx, 1:7] * float(np.float32(scale))
    dd = np.exp(arg)
    edd = (ULP2 + 1 + np.abs(arg)) * U * dd                # expf: 4 | the product's rounding moves the argument by |arg| U: |arg| | (+1 spare for the min side)
    lo, hi = dd[:, 0::2], dd[:, 1::2]
    elo, ehi = edd[:, 0::2], edd[:, 1::2]
    if R == 6:
        boxes = np.concatenate([pt - lo, pt + hi], 1)
        bound = np.concatenate([ept + elo + U * (np.abs(pt) + lo), ept + ehi + U * (np.abs(pt) + hi)], 1)      # point | distance | the final add: 1
    else:
        alpha = ho[idx, 7]
        sh = (hi - lo) / 2
        esh = (ehi + elo + U * (hi + lo)) / 2                                              # the difference: 1, the halving exact
        c, s = np.cos(alpha), np.sin(alpha)
        rx, ry = sh[:, 0] * c + sh[:, 1] * s, -sh[:, 0] * s + sh[:, 1] * c
        # each product: the shift's error, sinf / cosf at 4 U absolute (|.| <= 1), the product's rounding: 1; the sum: 1
        erot = esh[:, 0] + esh[:, 1] + (np.abs(sh[:, 0]) + np.abs(sh[:, 1])) * (ULP2 + 1 + 1) * U
        boxes = np.concatenate([np.stack([pt[:, 0] + rx, pt[:, 1] + ry, pt[:, 2] + sh[:, 2]], 1), lo + hi, alpha[:, None]], 1)
        bound = np.concatenate([np.stack([ept[:, 0] + erot + U * (np.abs(pt[:, 0]) + np.abs(rx)), ept[:, 1] + erot + U * (np.abs(pt[:, 1]) + np.abs(ry)),
                                          ept[:, 2] + esh[:, 2] + U * (np.abs(pt[:, 2]) + np.abs(sh[:, 2]))], 1),
                                elo + ehi + U * (lo + hi), np.zeros((k, 1))], 1)
    sc = scores[idx]
    return dict(k=k, idx=idx, boxes=boxes, box_bound=bound * SECOND + TINY, scores=sc, score_bound=K_FCOS_SCORE * U * SECOND * sc + TINY, margin=margin)


# ------------------------------------------------------------------------------------------------------------------ NMS forms
def multiclass_nms(boxes, scores, num_classes, score_thr, nms_thr, rotated, max_num):
    """box3d_multiclass_nms as include/imvoxel.h states it: per class the candidates with score > score_thr by descending score (ties:
    lower index), greedy NMS; the class-major concatenation when it fits max_num, otherwise the best max_num by score (ties: lower class,
    then earlier position).  scores [n, >= num_classes].  Returns (idx, labels, iou margin)."""
    sc = np.asarray(scores, np.float64)
    thr = float(np.float32(score_thr))
    idx, lab, ss, margin = [], [], [], np.inf
    for c in range(num_classes):
        cand = np.nonzero(sc[:, c] > thr)[0]
        cand = cand[np.lexsort((cand, -sc[cand, c]))]
        keep, m = greedy_nms(np.asarray(boxes)[cand], nms_thr, rotated)
        margin = min(margin, m)
        idx += list(cand[keep])
        lab += [c] * len(keep)
        ss += list(sc[cand[keep], c])
    idx, lab, ss = np.array(idx, np.int64), np.array(lab, np.int64), np.array(ss, np.float64)
    if idx.size > max_num:
        o = np.lexsort((np.arange(idx.size), -ss))[:max_num]
        idx, lab = idx[o], lab[o]
    return idx, lab, margin


def aligned_3d_nms(boxes, scores, classes, thresh):
    """aligned_3d_nms: descending score (ties: lower index first); a picked box removes every later box j with NOT(iou * same_class <= thresh).
    The rule for degenerate boxes, explicitly: where the IoU is NaN (0 / 0 of two zero-volume boxes, or a NaN corner) the product with
    same_class is NaN too, `NaN <= thresh` is false, and the box is removed WHATEVER its class.  Returns (picks, margin)."""
    b = np.asarray(boxes, np.float64).reshape(-1, 6)
    s = np.asarray(scores, np.float64)
    cl = np.asarray(classes)
    n = b.shape[0]
    thr = float(np.float32(thresh))
    order = np.lexsort((np.arange(n), -s))
    vol = (b[:, 3] - b[:, 0]) * (b[:, 4] - b[:, 1]) * (b[:, 5] - b[:, 2])
    removed = np.zeros(n, bool)
    pick, margin = [], np.inf
    for p, i in enumerate(order):
        if removed[i]:
            continue
        pick.append(i)
        rest = order[p + 1:]
        rest = rest[~removed[rest]]
        if rest.size == 0:
            continue
        with np.errstate(invalid='ignore', divide='ignore'):
            ext = np.maximum(0.0, np.fmin(b[i, 3:], b[rest, 3:]) - np.fmax(b[i, :3], b[rest, :3]))
            inter = ext.prod(1)
            iou = inter / (vol[i] + vol[rest] - inter) * (cl[rest] == cl[i])
        fin = np.isfinite(iou) & (cl[rest] == cl[i])
        if fin.any():
            margin = min(margin, float(np.abs(iou[fin] - thr).min()))
        removed[rest[~(iou <= thr)]] = True
    return np.array(pick, np.int64), margin


def indoor_tail_scannet(cand_boxes, cand_scores, score_thr, nms_thr, max_num):
    """One sample, the levels concatenated: boxes [K, 6] corners, scores [K, ncls].  Class maximum (first maximum) and label, score > thr,
    class-aware aligned_3d_nms, the first max_num, corners -> (centre x, y, BOTTOM z, sizes, yaw 0).  Returns (rows, bound, scores, labels, margin)."""
    b, s = np.asarray(cand_boxes, np.float64), np.asarray(cand_scores, np.float64)
    lab, best = s.argmax(1), s.max(1)
    sel = np.nonzero(best > float(np.float32(score_thr)))[0]
    pick, margin = aligned_3d_nms(b[sel], best[sel], lab[sel], nms_thr)
    pick = sel[pick][:max_num]
    c = b[pick]
    dz = c[:, 5] - c[:, 2]
    rows = np.stack([(c[:, 0] + c[:, 3]) / 2, (c[:, 1] + c[:, 4]) / 2, (c[:, 2] + c[:, 5]) / 2 + dz * -0.5, c[:, 3] - c[:, 0], c[:, 4] - c[:, 1], dz,
                     np.zeros(len(pick))], 1)
    ax, ay, az = np.abs(c[:, 0]) + np.abs(c[:, 3]), np.abs(c[:, 1]) + np.abs(c[:, 4]), np.abs(c[:, 2]) + np.abs(c[:, 5])
    # centre: the sum 1, halving exact | bottom z: the sum 1, dz 1 (halved), the final add 1 = 3 on |z1| + |z2| | sizes: 1
    bound = U * np.stack([ax, ay, 3 * az, ax, ay, az, np.zeros(len(pick))], 1) + TINY
    return rows, bound, best[pick], lab[pick], margin


def indoor_tail_sunrgbd(cand_boxes, cand_scores, score_thr, nms_thr, rotated, max_num):
    """One sample: boxes [K, 7] (cx, cy, cz, w, l, h, alpha), scores [K, ncls].  BEV boxes (x -+ w/2, y -+ l/2, alpha), multiclass_nms with
    max_num, rows (x, y, z - h/2, w, l, h, alpha).  Returns (rows, bound, scores, labels, margin)."""
    b, s = np.asarray(cand_boxes, np.float64), np.asarray(cand_scores, np.float64)
    bev = np.stack([b[:, 0] - b[:, 3] / 2, b[:, 1] - b[:, 4] / 2, b[:, 0] + b[:, 3] / 2, b[:, 1] + b[:, 4] / 2, b[:, 6]], 1)
    idx, lab, margin = multiclass_nms(bev, s, s.shape[1], score_thr, nms_thr, rotated, max_num)
    r = b[idx].copy()
    r[:, 2] = r[:, 2] + r[:, 5] * -0.5
    bound = np.zeros_like(r)
    bound[:, 2] = U * (np.abs(b[idx, 2]) + np.abs(b[idx, 5]) / 2) + TINY                   # the one add: 1
    return r, bound, s[idx, lab], lab, margin


# ------------------------------------------------------------------------------------------------------------------ checkers
def check_close(name, got, ref, bound):
    """|got - ref| <= bound elementwise, no NaN left from the pre-fill; returns the worst error / bound"""
    got, ref, bound = np.asarray(got, np.float64), np.asarray(ref, np.float64), np.asarray(bound, np.float64)
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    if got.size == 0:
        return 0.0
    assert np.isfinite(got).all(), f'{name}: {int((~np.isfinite(got)).sum())} values not written or not finite'
    err = np.abs(got - ref)
    ratio = np.where(err == 0, 0.0, err / np.maximum(bound, 1e-300))
    worst = float(ratio.max())
    at = np.unravel_index(int(ratio.argmax()), ratio.shape)
    assert worst <= 1.0, f'{name}: |got - ref| = {err[at]:.3e} is {worst:.2f} x the bound {bound[at]:.3e} at {at}'
    return worst


def check_same(name, got, ref):
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape and np.array_equal(got, ref), f'{name}: got {got.tolist()[:40]} expected {ref.tolist()[:40]}'


# ------------------------------------------------------------------------------------------------------------------ backends
class AnchorHeadDesc(C.Structure):              # ivx_anchor_head_desc
    _fields_ = [(n, C.c_int32) for n in ('B', 'H', 'W', 'CH', 'num_anchors', 'num_classes', 'cls_off', 'reg_off', 'dir_off', 'nms_pre', 'max_num',
                                         'use_rotate_nms', 'hw_transposed')] + [(n, C.c_float) for n in ('score_thr', 'nms_thr', 'dir_offset', 'dir_limit_offset')]


class IndoorTailDesc(C.Structure):              # ivx_indoor_tail_desc
    _fields_ = [('B', C.c_int32), ('n_levels', C.c_int32), ('k', C.c_int32 * 4), ('n_classes', C.c_int32), ('n_reg', C.c_int32),
                ('use_rotate_nms', C.c_int32), ('max_num', C.c_int32), ('score_thr', C.c_float), ('nms_thr', C.c_float)]


class HostBackend:
    """The entry points on host memory (the CPU restatement).  tests/test_gpu_tail_fp64.py has the device twin with the same methods."""
    name = 'cpu'
    AnchorHeadDesc, IndoorTailDesc = AnchorHeadDesc, IndoorTailDesc

    def __init__(self, L):
        self.L = L
        bind(L)
        self.stream = None

    def up(self, a):
        return np.ascontiguousarray(a).copy()

    def full(self, shape, dtype, fill):
        return np.full(shape, fill, dtype)

    def ptr(self, h, byte_offset=0):
        return C.c_void_p(h.ctypes.data + byte_offset) if h is not None else None

    def get(self, h):
        return h

    def ok(self, rc, what):
        assert rc == 0, f'{what}: {self.L.ivx_last_error().decode()}'

    def workspace(self, nbytes):
        raw = np.zeros(int(nbytes) + 512, np.uint8)
        off = -raw.ctypes.data % 256
        return raw, C.c_void_p(raw.ctypes.data + off)


def bind(L):
    """argument types of the tail's entry points (include/imvoxel.h), for a library loaded without them"""
    vp, i32, i64, f32 = C.c_void_p, C.c_int32, C.c_int64, C.c_float
    L.ivx_last_error.restype = C.c_char_p
    for name, res, args in [
            ('ivx_anchor_head_workspace_bytes', i64, [vp]),
            ('ivx_anchor_head_get_bboxes', C.c_int, [vp, vp, vp, vp, i64, vp, vp, vp, vp, vp, vp, vp, vp]),
            ('ivx_fcos_head_workspace_bytes', i64, [i32, i32, i32]),
            ('ivx_fcos_head_level_candidates', C.c_int, [vp, vp, vp, vp, f32] + [i32] * 12 + [vp, i64, vp, vp, vp, vp]),
            ('ivx_nms_workspace_bytes', i64, [i32]),
            ('ivx_nms_bev', C.c_int, [vp, i32, f32, i32, vp, i64, vp, vp, vp]),
            ('ivx_boxes_overlap_bev', C.c_int, [vp, i32, vp, i32, i32, vp, vp]),
            ('ivx_aligned_3d_nms', C.c_int, [vp, vp, vp, i32, f32, vp, vp, vp]),
            ('ivx_aligned_3d_nms_workspace_bytes', i64, [i32]),
            ('ivx_aligned_3d_nms_ws', C.c_int, [vp, vp, vp, i32, f32, vp, i64, vp, vp, vp]),
            ('ivx_multiclass_nms_workspace_bytes', i64, [i32, i32]),
            ('ivx_multiclass_nms_bev', C.c_int, [vp, vp, i32, i32, i32, f32, f32, i32, i32, vp, i64, vp, vp, vp, vp]),
            ('ivx_indoor_tail_workspace_bytes', i64, [vp]),
            ('ivx_indoor_tail_get_bboxes', C.c_int, [vp, vp, vp, vp, i64, vp, vp, vp, vp, vp])]:
        f = getattr(L, name)
        f.restype, f.argtypes = res, args


def _ws(be, nbytes, what):
    assert nbytes >= 0, what
    return be.workspace(max(int(nbytes), 256)) + (int(max(nbytes, 256)),)


# ------------------------------------------------------------------------------------------------------------------ rotated overlap
# Worst |C oracle - fp64| / min(area_a, area_b) of oracle.c_oracle.boxes_overlap_bev per configuration class, both argument orders, over
# overlap_case(cls, seed, na, nb) for the seeds of OVERLAP_SEEDS and the shapes of OVERLAP_SHAPES (585 class pairs per class).  Measured 2026-10-19 with
#   pytest -s tests/test_host_tail_fp64.py::test_overlap_oracle_measured
# which prints them and asserts measured <= constant <= max(2 x measured, 2^-22): the constants are the measurements rounded up.
OVERLAP_SLACK = 4.0
OVERLAP_SEEDS = (0, 1, 2)
OVERLAP_SHAPES = [(1, 1), (1, 65), (63, 64), (65, 3)]
OVERLAP_MEASURED = {
    'generic': 2.0e-6, 'right_angles': 3.2e-6, 'zero_angles': 3.7e-6,
    # collinear edges: 584 of the 585 pairs are below 4e-6; one pair, in one argument order, comes out 7 % too large (the 1e-5 margin of the in-box
    # test and the crossing test of nearly parallel edges collect a point that is no vertex) -- the reference's own algorithm, iou3d_kernel.cu:127-242
    'collinear': 2.7e-2,
    'shared_edge': 2.0 ** -22, 'touching_corner': 2.0 ** -22,          # measured exactly 0: the floor of one fp32 ulp of the area
    'contained_same_angle': 6.6e-6, 'contained_other_angle': 3.0e-5, 'quarter_turn': 4.7e-6, 'nearly_parallel': 3.7e-6, 'sliver': 5.2e-6,
    'thin': 1.8e-5, 'identical': 1.9e-6, 'far_origin': 1.6e-4,
}
OVERLAP_EXPECT = {'shared_edge': 'zero', 'touching_corner': 'zero', 'identical': 'area'}


def _xyxy(cx, cy, w, h, ang):
    return np.stack([cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2, ang], -1).astype(np.float32)


def overlap_class_pairs(cls, seed, m, small=None):
    """m pairs (a [m, 5], b [m, 5]) fp32 of a configuration class: boxes 0.5 .. 3.5 wide, centres within 20.  Only `small` different first
    boxes (pair t has the first box t % small), each with its own partner."""
    r = np.random.RandomState(1000 * seed + sum(map(ord, cls)))
    small = small or m
    rep = np.arange(m) % small
    cx, cy = r.uniform(-20, 20, small)[rep], r.uniform(-20, 20, small)[rep]
    w, h = r.uniform(0.5, 3.5, small)[rep], r.uniform(0.5, 3.5, small)[rep]
    ang = r.uniform(-np.pi, np.pi, small)[rep]
    w2, h2 = r.uniform(0.5, 3.5, m), r.uniform(0.5, 3.5, m)
    near = lambda s: (cx + r.uniform(-s, s, m), cy + r.uniform(-s, s, m))          # noqa: E731
    co, si = np.cos(ang), np.sin(ang)
    if cls == 'generic':
        x2, y2 = near(2.0)
        return _xyxy(cx, cy, w, h, ang), _xyxy(x2, y2, w2, h2, r.uniform(-np.pi, np.pi, m))
    if cls == 'right_angles':
        q = np.float32(np.pi / 2)
        x2, y2 = near(2.0)
        return _xyxy(cx, cy, w, h, r.randint(-3, 4, small)[rep] * q), _xyxy(x2, y2, w2, h2, r.randint(-3, 4, m) * q)
    if cls == 'zero_angles':
        x2, y2 = near(2.0)
        return _xyxy(cx, cy, w, h, 0 * ang), _xyxy(x2, y2, w2, h2, 0 * ang)
    if cls == 'collinear':                      # same angle, same width, shifted along the box's own x axis
        t = r.uniform(0.1, 0.9, m) * w
        return _xyxy(cx, cy, w, h, ang), _xyxy(cx + t * co, cy - t * si, w, h, ang)
    if cls == 'shared_edge':                    # axis-aligned, exactly representable: b begins where a ends, on one of the four sides
        cx, cy, w, h = np.round(cx), np.round(cy), np.round(w * 2) / 2 + 0.5, np.round(h * 2) / 2 + 0.5
        sx, sy = np.array([1, -1, 0, 0])[r.randint(0, 4, m)], 0
        sy = np.where(sx == 0, r.choice([-1, 1], m), 0)
        return _xyxy(cx, cy, w, h, 0 * ang), _xyxy(cx + sx * w, cy + sy * h, w, h, 0 * ang)
    if cls == 'touching_corner':
        cx, cy, w, h = np.round(cx), np.round(cy), np.round(w * 2) / 2 + 0.5, np.round(h * 2) / 2 + 0.5
        return _xyxy(cx, cy, w, h, 0 * ang), _xyxy(cx + r.choice([-1, 1], m) * w, cy + r.choice([-1, 1], m) * h, w, h, 0 * ang)
    if cls == 'contained_same_angle':
        f = r.uniform(0.2, 0.4, m)
        return _xyxy(cx, cy, w + 1, h + 1, ang), _xyxy(cx + f * co - 0.1 * si, cy - f * si - 0.1 * co, w * f, h * f, ang)
    if cls == 'contained_other_angle':          # b's half diagonal is below a's half extent
        s = np.minimum(w, h) * r.uniform(0.1, 0.3, m)
        return _xyxy(cx, cy, w, h, ang), _xyxy(cx, cy, s, s * 0.8, r.uniform(-np.pi, np.pi, m))
    if cls == 'quarter_turn':
        return _xyxy(cx, cy, w, h, ang), _xyxy(cx, cy, w, h, ang + np.float32(np.pi / 2))
    if cls == 'nearly_parallel':
        x2, y2 = near(0.5)
        return _xyxy(cx, cy, w, h, ang), _xyxy(x2, y2, w2, h2, ang + r.choice([-1, 1], m) * 1e-4)
    if cls == 'sliver':                         # overlap 1e-3 of the width
        return _xyxy(cx, cy, w, h, ang), _xyxy(cx + (1 - 1e-3) * w * co, cy - (1 - 1e-3) * w * si, w, h, ang + 0.2 * r.uniform(-1, 1, m) * 1e-3)
    if cls == 'thin':
        x2, y2 = near(0.3)
        return _xyxy(cx, cy, w, 0.01 + 0 * h, ang), _xyxy(x2, y2, 0.01 + 0 * w, h2, r.uniform(-np.pi, np.pi, m))
    if cls == 'identical':
        a = _xyxy(cx, cy, w, h, ang)
        return a, a.copy()
    if cls == 'far_origin':
        x2, y2 = near(2.0)
        return _xyxy(cx + 1000, cy + 1000, w, h, ang), _xyxy(x2 + 1000, y2 + 1000, w2, h2, r.uniform(-np.pi, np.pi, m))
    raise KeyError(cls)


OVERLAP_CLASSES = ['generic', 'right_angles', 'zero_angles', 'collinear', 'shared_edge', 'touching_corner', 'contained_same_angle',
                   'contained_other_angle', 'quarter_turn', 'nearly_parallel', 'sliver', 'thin', 'identical', 'far_origin']


def overlap_case(cls, seed, na, nb):
    """a [na, 5], b [nb, 5] and the index lists (i, j) of the max(na, nb) class pairs among the na x nb entries: entry (t % na, t % nb) for every t.
    The other entries are whatever comes and are not checked against the class bound."""
    m, small = max(na, nb), min(na, nb)
    first, partner = overlap_class_pairs(cls, seed * 7 + na + nb, m, small)
    a, b = (first[:small], partner) if na <= nb else (partner, first[:small])
    return a, b, (np.arange(m) % na, np.arange(m) % nb)


def overlap_measure(fn, cls, seed, na, nb):
    """worst |fn - fp64| / min area over the class pairs of the case, both argument orders; fn(a, b) -> [na, nb] areas"""
    a, b, (i, j) = overlap_case(cls, seed, na, nb)
    ref = overlap_matrix(a, b)
    amin = np.minimum(areas(a)[:, None], areas(b)[None, :])
    g1, g2 = np.asarray(fn(a, b), np.float64), np.asarray(fn(b, a), np.float64).T
    assert np.isfinite(g1).all() and np.isfinite(g2).all(), (cls, 'unwritten or non-finite overlap')
    e = np.maximum(np.abs(g1 - ref), np.abs(g2 - ref)) / amin
    exp = OVERLAP_EXPECT.get(cls)
    if exp == 'zero':
        assert np.all(ref[i, j] <= 1e-12), cls
    if exp == 'area':
        assert np.allclose(ref[i, j], areas(a)[i], rtol=1e-12), cls
    return float(e[i, j].max()), ref, amin, (i, j)


def run_overlap(be, cls):
    """ivx_boxes_overlap_bev, both iou values, every shape of OVERLAP_SHAPES, against overlap_matrix within OVERLAP_SLACK x OVERLAP_MEASURED[cls]
    of the smaller area on the class pairs; the IoU with the same bound propagated through so / max(sa + sb - so, 1e-8).  Returns the worst ratio."""
    L, worst = be.L, 0.0
    allow = OVERLAP_SLACK * OVERLAP_MEASURED[cls]

    def call(iou):
        def fn(a, b):
            da, db = be.up(a), be.up(b)
            out = be.full((a.shape[0], b.shape[0]), np.float32, np.nan)
            be.ok(L.ivx_boxes_overlap_bev(be.ptr(da), a.shape[0], be.ptr(db), b.shape[0], iou, be.ptr(out), be.stream), 'ivx_boxes_overlap_bev')
            return be.get(out)
        return fn
    for seed in OVERLAP_SEEDS:
        for na, nb in OVERLAP_SHAPES:
            e, ref, amin, (i, j) = overlap_measure(call(0), cls, seed, na, nb)
            assert e <= allow, f'{be.name} overlap {cls} {na}x{nb}: error / min area {e:.3e} above {OVERLAP_SLACK} x {OVERLAP_MEASURED[cls]:.1e}'
            worst = max(worst, e / allow)
            a, b, _ = overlap_case(cls, seed, na, nb)
            sa, sb = areas(a)[:, None], areas(b)[None, :]
            un = np.maximum(sa + sb - ref, 1e-8)
            iref = ref / un
            # d(so / (S - so)) = S / (S - so)^2 d so, plus the five roundings of the areas, the sum, the difference and the quotient
            ibound = (allow * amin) * (sa + sb) / un ** 2 + 8 * U * iref + TINY
            g1, g2 = np.asarray(call(1)(a, b), np.float64), np.asarray(call(1)(b, a), np.float64).T
            r = np.maximum(np.abs(g1 - iref), np.abs(g2 - iref))[i, j] / ibound[i, j]
            assert r.max() <= 1.0, f'{be.name} iou {cls} {na}x{nb}: {r.max():.2f} x the propagated bound'
            worst = max(worst, float(r.max()))
    return worst


def robust(build, margin_of, what, tries=64):
    """The first build(attempt), attempt = 0, 1, ..., whose reference margin is at least twice the required one.  The choice is made by the fp64
    reference alone, never by the code under test: an input whose answer the reference cannot defend is not an input of this suite."""
    for attempt in range(tries):
        x = build(attempt)
        if margin_of(x) >= 2 * IOU_MARGIN:
            return x
    raise AssertionError(f'{what}: no robust input in {tries} tries')


# ------------------------------------------------------------------------------------------------------------------ ivx_nms_bev
NMS_SIZES = [0, 1, 2, 63, 64, 65, 128, 129, 300]
NMS_THRS = [0.1, 0.7]


def _rand_boxes(r, n, spread, lo=0.5, hi=3.5):
    return _xyxy(r.uniform(-spread, spread, n), r.uniform(-spread, spread, n), r.uniform(lo, hi, n), r.uniform(lo, hi, n), r.uniform(-np.pi, np.pi, n))


def nms_cases(rotated):
    """(name, boxes [n, 5] fp32 in descending score, thr, expected kept or None).  The seeds were chosen on the CPU so that the reference's
    decision margin is at least IOU_MARGIN; both tests assert it."""
    out = []
    for thr in NMS_THRS:
        s = 0.6 if thr < 0.5 else 0.1                 # chain shift in widths: IoU(i, i+1) = (1-s)/(1+s) above thr, IoU(i, i+2) below it
        for n in NMS_SIZES:
            r = np.random.RandomState(n * 10 + int(thr * 10) + (3 if rotated else 0))
            one = _xyxy(np.array([1.5]), np.array([-2.0]), np.array([2.0]), np.array([1.25]), np.array([0.4]))
            out.append((f'identical n{n} thr{thr}', np.repeat(one, n, 0), thr, np.arange(min(n, 1))))
            g = np.arange(n)
            out.append((f'disjoint n{n} thr{thr}', _xyxy(5.0 * (g % 17), 5.0 * (g // 17), r.uniform(0.5, 3.5, n), r.uniform(0.5, 3.5, n),
                                                         r.uniform(-np.pi, np.pi, n)), thr, g))
            seed0 = n * 10 + int(thr * 10) + (3 if rotated else 0)
            out.append((f'random n{n} thr{thr}', robust(lambda t: _rand_boxes(np.random.RandomState(seed0 + 1009 * t), n, 0.5 + 1.2 * np.sqrt(n)),
                                                        lambda bx: greedy_nms(bx, thr, rotated)[1], f'random nms n{n}'), thr, None))
            if n >= 65:
                # disjoint boxes except chains across the word boundaries: box 63 suppresses 64, which would have suppressed 65; 65 does not
                # overlap 63 beyond thr and is kept (the same at 127 / 128 / 129); box 5 overlaps only a box of lower score, the last one
                ang = 0.3 if rotated else 0.0
                b = _xyxy(6.0 * (g % 17), 6.0 * (g // 17) + 10, 2.0 + 0 * g, 1.0 + 0 * g, ang + 0 * g).astype(np.float64)
                expect = np.ones(n, bool)
                for first in (63, 127):
                    if first + 2 < n:
                        for q in (1, 2):
                            b[first + q] = b[first]
                            dx, dy = (q * s * 2.0 * np.cos(ang), -q * s * 2.0 * np.sin(ang)) if rotated else (q * s * 2.0, 0.0)
                            b[first + q, [0, 2]] += dx
                            b[first + q, [1, 3]] += dy
                            b[first + q, 4] = ang + (0.01 * q if rotated else 0.0)
                        expect[first + 1] = False
                b[n - 1] = b[5]                                     # box 5 overlaps only a box of lower score (the last): 5 is kept, the last removed
                b[n - 1, [0, 2]] += 0.05
                expect[n - 1] = False
                out.append((f'chain n{n} thr{thr}', b.astype(np.float32), thr, np.nonzero(expect)[0]))
    if not rotated:
        # 2 x 2 boxes with centres on a lattice of 0.5: the IoU takes a few values, the nearest to 0.5 are 0.391 and 0.6
        r = np.random.RandomState(4097)
        n = 4097
        out.append(('lattice n4097 thr0.5 (the LDS removal words)', _xyxy(0.5 * r.randint(0, 90, n), 0.5 * r.randint(0, 90, n), 2.0 + np.zeros(n),
                                                                            2.0 + np.zeros(n), np.zeros(n)), 0.5, None))
    return out


def run_nms(be, rotated):
    L, smallest = be.L, np.inf
    for name, boxes, thr, expect in nms_cases(rotated):
        n = boxes.shape[0]
        keep_ref, margin = greedy_nms(boxes, thr, rotated)
        assert margin >= IOU_MARGIN, f'{name}: the reference decides at |IoU - thr| = {margin:.2e}; choose another seed'
        smallest = min(smallest, margin)
        if expect is not None:
            check_same(f'{name} (reference against the construction)', keep_ref, expect)
        db = be.up(boxes if n else np.zeros((1, 5), np.float32))
        keep, num = be.full((max(n, 1),), np.int64, -7), be.full((1,), np.int32, -7)
        nb = L.ivx_nms_workspace_bytes(n)
        raw, ws, nb = _ws(be, nb, 'ivx_nms_workspace_bytes')
        be.ok(L.ivx_nms_bev(be.ptr(db), n, thr, int(rotated), ws, nb, be.ptr(keep), be.ptr(num), be.stream), 'ivx_nms_bev')
        k = int(be.get(num)[0])
        tag = f'{be.name} nms {"rotated" if rotated else "axis"} {name}'
        assert k == keep_ref.size, f'{tag}: kept {k}, expected {keep_ref.size}'
        check_same(tag, be.get(keep)[:k], keep_ref)
    return smallest


# ------------------------------------------------------------------------------------------------------------------ anchor head
def grid_logits(r, n, lo=-4.0, hi=3.0):
    """a seeded permutation of a grid of n logits: unequal sigmoid scores differ by step * sigmoid(-hi) >= SCORE_MARGIN relative"""
    step = (hi - lo) / max(n, 2)
    assert step * sigmoid(-hi) >= 1.5 * SCORE_MARGIN
    return r.permutation(lo + step * np.arange(n)).astype(np.float32)


def anchor_layouts(A):
    """(name, CH, cls_off, reg_off, dir_off): the usual cls | reg | dir, and dir | pad | cls | pad | reg | pad with CH a multiple of 8"""
    usual = ('usual', 10 * A, 0, A, 8 * A)
    d0, c0, r0 = 0, 2 * A + 3, 2 * A + 3 + A + 2
    ch = (r0 + 7 * A + 1 + 7) // 8 * 8
    return [usual, ('padded', ch, c0, r0, d0)]


def anchor_cases():
    """dicts of descriptor fields plus 'seed', 'thr_pos', 'layout'.  Every listed value of every parameter occurs; the product is not taken."""
    cases = []
    grids = [(1, 1, 1), (3, 7, 3), (4, 8, 2), (5, 13, 1), (9, 11, 2)]
    dirs = [(0.0, 1.0), (np.pi / 4, 0.0), (0.0, 0.5)]
    i = 0
    for (H, W, A) in grids:
        n = H * W * A
        for pre in sorted({1, max(n - 1, 1), n, n + 5}):
            for thr_pos in ('below', 'above', 'middle', 'half'):
                lay = i % 2
                cases.append(dict(H=H, W=W, num_anchors=A, B=(3 if i % 3 == 0 else 1), nms_pre=pre, hw_transposed=(i // 2) % 2, layout=lay,
                                  use_rotate_nms=(i // 3) % 2, thr_pos=thr_pos, max_sel=('one', 'fewer', 'more')[i % 3],
                                  nms_thr=(0.1, 0.5, 0.7)[(i // 5) % 3], dir=dirs[i % 3], seed=i))
                i += 1
    return cases


def anchor_sample(c, b, attempt):
    """head_out [H*W, CH] of sample b in (y, x) order"""
    H, W, A = c['H'], c['W'], c['num_anchors']
    n = H * W * A
    r = np.random.RandomState(100 + 10 * c['seed'] + b + 1009 * attempt)
    _, CH, cls_off, reg_off, dir_off = anchor_layouts(A)[c['layout']]
    ho = r.uniform(-9, 9, (H * W, CH)).astype(np.float32)                # the padding channels hold noise of the size of real logits
    lg = grid_logits(r, n)
    if n >= 4:
        p = r.choice(n, 4, replace=False)
        lg[p[1]] = lg[p[0]]                                               # a bit-equal pair: the lower index first
        lg[p[2]] = 0.0                                                    # sigmoid(0) is exactly 0.5 in fp32 and fp64
        lg[p[3]] = lg[np.argmax(lg)]                                      # a tie at the very top
    ho[:, cls_off:cls_off + A] = lg.reshape(H * W, A)
    reg = r.uniform(-0.6, 0.6, (n, 7))
    reg[:, :2] *= 0.5
    reg[:, 6] = r.uniform(-8.5, 8.5, n)                                   # yaw deltas that put rg beyond +- 2 pi
    ho[:, reg_off:reg_off + 7 * A] = reg.reshape(H * W, 7 * A).astype(np.float32)
    dd = r.uniform(-2, 2, (n, 2)).astype(np.float32)
    dd[::5, 1] = dd[::5, 0]                                               # d0 == d1: direction 0
    ho[:, dir_off:dir_off + 2 * A] = dd.reshape(H * W, 2 * A)
    return ho


def anchor_inputs(c):
    """-> (head_out [B, H, W, CH] in (y, x) order, anchors [n, 7], descriptor dict, the references per sample).  The memory layout (hw_transposed)
    is the driver's.  Every sample is the first of its seeds whose reference decisions are robust (robust())."""
    H, W, A, B = c['H'], c['W'], c['num_anchors'], c['B']
    n = H * W * A
    _, CH, cls_off, reg_off, dir_off = anchor_layouts(A)[c['layout']]
    # anchors: flat order y, x, (size, rotation); two sizes and two rotations, so diag, ha and ra vary per anchor
    sizes = [(1.6, 3.9, 1.56), (0.6, 0.8, 1.73)]
    rots = [0.0, 1.57]
    base = {1: [(sizes[0], rots[0])], 2: [(sizes[0], rots[0]), (sizes[1], rots[1])], 3: [(sizes[0], rots[0]), (sizes[0], rots[1]), (sizes[1], rots[0])]}[A]
    an = np.zeros((H, W, A, 7), np.float32)
    for y in range(H):
        for x in range(W):
            for a, (s, ro) in enumerate(base):
                an[y, x, a] = (2.2 * x - 3.0, 2.6 * y + 2.0, -1.78 + 0.05 * a, s[0], s[1], s[2], ro)
    an = an.reshape(n, 7)
    desc = dict(B=B, H=H, W=W, CH=CH, num_anchors=A, num_classes=1, cls_off=cls_off, reg_off=reg_off, dir_off=dir_off, nms_pre=c['nms_pre'],
                use_rotate_nms=c['use_rotate_nms'], hw_transposed=c['hw_transposed'], nms_thr=c['nms_thr'], dir_offset=float(np.float32(c['dir'][0])),
                dir_limit_offset=c['dir'][1])

    def with_thr(ho0):
        sc = np.sort(sigmoid(ho0[:, cls_off:cls_off + A].reshape(n)))[::-1][:min(c['nms_pre'], n)]
        gaps = [i for i in range(1, len(sc)) if sc[i - 1] > sc[i] and abs(sc[i] - 0.5) > 0.01 and abs(sc[i - 1] - 0.5) > 0.01]
        i = min(gaps, key=lambda i: abs(i - len(sc) // 2)) if gaps else 0          # between the two unequal neighbours nearest to the middle
        mid = (sc[i - 1] + sc[i]) / 2 if gaps else sc[0] * 0.9
        return dict(desc, score_thr=float(np.float32({'below': 0.001, 'above': 0.999, 'half': 0.5, 'middle': mid}[c['thr_pos']])))
    margin = lambda rf: min(rf['iou_margin'], rf['yaw_margin'])            # noqa: E731
    ho0, d0 = robust(lambda t: (lambda h: (h, with_thr(h)))(anchor_sample(c, 0, t)),
                     lambda x: margin(anchor_tail(x[0], an, dict(x[1], max_num=1 << 20))), f'anchor head {c} sample 0')
    kept0 = len(anchor_tail(ho0, an, dict(d0, max_num=1 << 20))['keep'])
    desc = dict(d0, max_num={'one': 1, 'fewer': max(kept0 - 1, 1), 'more': kept0 + 3}[c['max_sel']])
    hos = [ho0] + [robust(lambda t: anchor_sample(c, b, t), lambda h: margin(anchor_tail(h, an, dict(desc, max_num=1 << 20))), f'anchor head {c} sample {b}')
                   for b in range(1, B)]
    return np.stack(hos).reshape(B, H, W, CH), an, desc, [anchor_tail(h, an, desc) for h in hos]


def run_anchor_head(be):
    """Every case of anchor_cases() through ivx_anchor_head_get_bboxes with the candidate outputs on.  Returns (worst ratio, margins)."""
    L, worst = be.L, 0.0
    marg = dict(score=np.inf, thr=np.inf, iou=np.inf, yaw=np.inf)
    seen_zero = seen_tie = 0
    for c in anchor_cases():
        ho, an, d, refs = anchor_inputs(c)
        B, H, W, CH = ho.shape
        P = d['nms_pre']
        M = d['max_num']
        mem = np.ascontiguousarray(ho.transpose(0, 2, 1, 3)) if d['hw_transposed'] else ho
        desc = be.AnchorHeadDesc(**d)
        raw, ws, nb = _ws(be, L.ivx_anchor_head_workspace_bytes(C.byref(desc)), 'ivx_anchor_head_workspace_bytes')
        dh, da = be.up(mem), be.up(an)
        ob, os_, ol, oc = be.full((B, M, 7), np.float32, np.nan), be.full((B, M), np.float32, np.nan), be.full((B, M), np.int64, -7), be.full((B,), np.int32, -7)
        ci, cb, cs = be.full((B, P), np.int64, -7), be.full((B, P, 7), np.float32, np.nan), be.full((B, P), np.float32, np.nan)
        be.ok(L.ivx_anchor_head_get_bboxes(C.byref(desc), be.ptr(dh), be.ptr(da), ws, nb, be.ptr(ob), be.ptr(os_), be.ptr(ol), be.ptr(oc), be.ptr(ci),
                                           be.ptr(cb), be.ptr(cs), be.stream), 'ivx_anchor_head_get_bboxes')
        ob, os_, ol, oc, ci, cb, cs = (be.get(t) for t in (ob, os_, ol, oc, ci, cb, cs))
        for b, rf in enumerate(refs):
            tag = f'{be.name} anchor head case {c} sample {b}'
            k = rf['k']
            assert rf['score_margin'] >= SCORE_MARGIN and rf['thr_margin'] >= SCORE_MARGIN, (tag, rf['score_margin'], rf['thr_margin'])
            assert rf['iou_margin'] >= IOU_MARGIN, f'{tag}: the reference decides at |IoU - thr| = {rf["iou_margin"]:.2e}; choose another seed'
            assert rf['yaw_margin'] >= YAW_MARGIN, f'{tag}: a fixed-up yaw {rf["yaw_margin"]:.2e} from a period boundary; choose another seed'
            for key, v in (('score', rf['score_margin']), ('thr', rf['thr_margin']), ('iou', rf['iou_margin']), ('yaw', rf['yaw_margin'])):
                marg[key] = min(marg[key], v)
            check_same(tag + ' candidate indices', ci[b], np.concatenate([rf['cand_idx'], np.full(P - k, -1, np.int64)]))
            worst = max(worst, check_close(tag + ' candidate boxes', cb[b, :k], rf['cand_boxes'], rf['cand_bound']))
            worst = max(worst, check_close(tag + ' candidate scores', cs[b, :k], rf['cand_scores'], rf['score_bound']))
            assert not cb[b, k:].any() and not cs[b, k:].any(), tag + ': candidate rows beyond k must be zero'
            cnt = len(rf['keep'])
            assert int(oc[b]) == cnt, f'{tag}: count {int(oc[b])}, expected {cnt}'
            # which candidates were kept: the output scores are copies of the candidate scores, whose indices were checked above
            worst = max(worst, check_close(tag + ' kept boxes', ob[b, :cnt], rf['out_boxes'], rf['out_bound']))
            worst = max(worst, check_close(tag + ' kept scores', os_[b, :cnt], rf['out_scores'], rf['score_bound'][rf['keep']]))
            check_same(tag + ' kept candidates (by score bits)', os_[b, :cnt].view(np.uint32), cs[b, rf['keep']].view(np.uint32))
            assert not ob[b, cnt:].any() and not os_[b, cnt:].any(), tag + ': rows beyond count must be zero'
            check_same(tag + ' labels', ol[b], np.zeros(M, np.int64))
            seen_zero += cnt == 0
            seen_tie += int((rf['cand_scores'][:-1] == rf['cand_scores'][1:]).any()) if k > 1 else 0
    assert seen_zero >= 5 and seen_tie >= 5, 'the cases must include empty results and bit-equal candidate scores'
    return worst, marg


# ------------------------------------------------------------------------------------------------------------------ FCOS level candidates
def _call_fcos(be, ho, valid0, vs, no, scale, ncls, R, level, nms_pre):
    """ho [B, nx, ny, nz, CH] fp32, valid0 [B, X, Y, Z] u8 -> (boxes [B, k, R], scores [B, k, ncls], count [B])"""
    L = be.L
    B, nx, ny, nz, CH = ho.shape
    X, Y, Z = valid0.shape[1:]
    n = nx * ny * nz
    k = nms_pre if 0 < nms_pre < n else n
    raw, ws, nb = _ws(be, L.ivx_fcos_head_workspace_bytes(B, n, nms_pre), 'ivx_fcos_head_workspace_bytes')
    dh, dv, dvs, dno = be.up(ho), be.up(valid0), be.up(np.asarray(vs, np.float32)), be.up(np.asarray(no, np.float32))
    cb, cs, cc = be.full((B, k, R), np.float32, np.nan), be.full((B, k, ncls), np.float32, np.nan), be.full((B,), np.int32, -7)
    be.ok(L.ivx_fcos_head_level_candidates(be.ptr(dh), be.ptr(dv), be.ptr(dvs), be.ptr(dno), float(np.float32(scale)), B, nx, ny, nz, CH, ncls, R, level,
                                           X, Y, Z, nms_pre, ws, nb, be.ptr(cb), be.ptr(cs), be.ptr(cc), be.stream), 'ivx_fcos_head_level_candidates')
    return be.get(cb), be.get(cs), be.get(cc)


def _check_fcos(be, tag, ho, valid0, vs, no, scale, ncls, R, level, nms_pre):
    cb, cs, cc = _call_fcos(be, ho, valid0, vs, no, scale, ncls, R, level, nms_pre)
    worst, margin = 0.0, np.inf
    for b in range(ho.shape[0]):
        rf = fcos_level_candidates(ho[b], valid0[b], vs[b], no[b], scale, ncls, R, level, nms_pre)
        assert rf['margin'] >= SCORE_MARGIN, f'{tag}: the reference orders at a relative score gap of {rf["margin"]:.2e}'
        margin = min(margin, rf['margin'])
        assert int(cc[b]) == rf['k'], (tag, int(cc[b]), rf['k'])
        # the candidate list holds no index: the boxes identify the voxel (the points differ by a voxel, the bound is rounding level)
        worst = max(worst, check_close(f'{tag} sample {b} boxes', cb[b], rf['boxes'], rf['box_bound']))
        worst = max(worst, check_close(f'{tag} sample {b} scores', cs[b], rf['scores'], rf['score_bound']))
    return worst, margin


TOPK_GRIDS = [(43, 127, 3), (32, 32, 16)]                 # n = 16383 and 16384: either side of the switch to the histogram form
TOPK_KS = [1, 64, 1000]
TOPK_PATTERNS = ['spread', 'one_bin', 'equal_block_at_cut', 'equal_flood_at_cut']


def topk_logits(pattern, n, k, seed):
    """class logits [n] for centerness logit 0 (sigmoid exactly 0.5: score = sigmoid(cls) / 2).  The first k + 40 of the sorted list are a grid
    with relative score gaps >= SCORE_MARGIN (or deliberate bit-equal blocks); what lies below may repeat values, it decides nothing."""
    r = np.random.RandomState(seed)
    top = k + 40
    if pattern == 'one_bin':                 # the first radix level bins key >> 21: scores in [0.25, 0.3125), i.e. logits in [0, 0.51)
        head = 0.5 - 3.2e-4 * np.arange(top)
        tail = r.choice(0.005 * np.arange(20), n - top)
    else:
        head = 3.0 - (5.0 / top) * np.arange(top)
        tail = r.choice(-8.0 + 0.025 * np.arange(200), n - top)
    if pattern == 'equal_block_at_cut':
        lo = max(k - 20, 0)
        head[lo:k + 20] = head[lo]
    v = np.concatenate([head, tail])
    if pattern == 'equal_flood_at_cut':      # more than 8192 bit-equal scores at the cut: the compacted list overflows its capacity
        v[k // 2:k // 2 + 9000] = v[k // 2]
    return r.permutation(v).astype(np.float32)


def run_fcos_topk(be, grid):
    worst, margin = 0.0, np.inf
    nx, ny, nz = grid
    n = nx * ny * nz
    for pattern in TOPK_PATTERNS:
        for k in TOPK_KS:
            ho = np.zeros((1, nx, ny, nz, 8), np.float32)
            r = np.random.RandomState(k)
            ho[..., 1:7] = r.uniform(-1, 1, (1, nx, ny, nz, 6))
            ho[..., 7] = topk_logits(pattern, n, k, seed=n + k).reshape(1, nx, ny, nz)
            valid0 = np.ones((1, nx, ny, nz), np.uint8)
            vs, no = np.array([[0.16, 0.16, 0.2]], np.float32), np.array([[-3.2, -0.1, -1.3]], np.float32)
            w, m = _check_fcos(be, f'{be.name} fcos top-k n{n} k{k} {pattern}', ho, valid0, vs, no, 1.0, 1, 6, 0, k)
            worst, margin = max(worst, w), min(margin, m)
    return worst, margin


def pooled_mask_probe(X, Y, Z, level, seed):
    """a level-0 mask whose pooled cells see 0, 4, 5 and 8 set voxels (cycled over the cells; which 4 / 5 of the 8 are random), noise elsewhere"""
    r = np.random.RandomState(seed)
    v = (r.uniform(size=(X, Y, Z)) < 0.5).astype(np.uint8)
    h, st = (1 << (level - 1)) - 1, 1 << level
    counts = []
    for ci, (i, j, l) in enumerate(np.ndindex(X >> level, Y >> level, Z >> level)):
        want = (0, 4, 5, 8, 3, 6)[ci % 6]
        bits = np.zeros(8, np.uint8)
        bits[r.permutation(8)[:want]] = 1
        v[i * st + h:i * st + h + 2, j * st + h:j * st + h + 2, l * st + h:l * st + h + 2] = bits.reshape(2, 2, 2)
        counts.append(want)
    return v, counts


# (level-0 grid, level, R, ncls, CH, scale, nms_pre as a function of n)
FCOS_CASES = [((12, 10, 6), 0, 6, 3, 10, 1.0, lambda n: n + 5), ((12, 10, 6), 0, 7, 2, 16, 0.75, lambda n: 100),
              ((12, 10, 6), 1, 6, 2, 12, 1.3, lambda n: n), ((12, 10, 6), 1, 7, 10, 18, 0.5, lambda n: n - 1),
              ((12, 8, 4), 2, 6, 1, 8, 1.1, lambda n: 4), ((12, 8, 4), 2, 7, 3, 11, 1.0, lambda n: n + 1),
              ((16, 24, 8), 1, 7, 2, 10, 0.9, lambda n: 65), ((16, 24, 8), 2, 6, 18, 25, 1.2, lambda n: 7)]


def run_fcos_levels(be):
    worst, margin = 0.0, np.inf
    for ci, ((X, Y, Z), level, R, ncls, CH, scale, pre) in enumerate(FCOS_CASES):
        nx, ny, nz = X >> level, Y >> level, Z >> level
        n, B = nx * ny * nz, 2
        r = np.random.RandomState(50 + ci)
        ho = r.uniform(-1.5, 1.5, (B, nx, ny, nz, CH)).astype(np.float32)
        for b in range(B):
            # the key sigmoid(cls) * sigmoid(centerness) of a voxel is a seeded permutation of a geometric grid 0.02 .. 0.25 (ratio >= 1 + 10 SCORE_MARGIN):
            # the centerness logit is drawn, the logit of one class follows from it; the other classes sit far below; a few voxels are copies (ties)
            assert np.log(12.5) / n >= 10 * SCORE_MARGIN
            key = r.permutation(0.02 * 12.5 ** (np.arange(n) / n))
            ctr = r.choice([-1.0, 0.0, 0.5, 2.0], n)
            q = key / sigmoid(ctr)
            lg = np.log(q / (1 - q))
            rows = ho[b].reshape(n, CH)
            rows[:, 0] = ctr
            rows[:, 1 + R:1 + R + ncls] = r.uniform(-9, -7, (n, ncls))
            rows[np.arange(n), 1 + R + r.randint(0, ncls, n)] = lg
            if n >= 8:
                p = r.choice(n, 8, replace=False)
                rows[p[4:], 0], rows[p[4:], 1 + R:1 + R + ncls] = rows[p[:4], 0], rows[p[:4], 1 + R:1 + R + ncls]
        if R == 7:
            ho[..., 7] = r.uniform(-3.5, 3.5, (B, nx, ny, nz))
        masks = [pooled_mask_probe(X, Y, Z, level, 9 * ci + b) if level else ((r.uniform(size=(X, Y, Z)) < 0.7).astype(np.uint8), None) for b in range(B)]
        valid0 = np.stack([m[0] for m in masks])
        for b in range(B):
            if level:
                pv = pooled_valid(valid0[b], level).reshape(-1)
                assert {0, 4, 5, 8} <= set(masks[b][1]) and np.array_equal(pv, np.array(masks[b][1]) >= 5), 'the probe mask and the pooling rule'
        vs = np.array([[0.16, 0.2, 0.24], [0.08, 0.1, 0.3]], np.float32) * (1 << level)              # per sample, different
        no = np.array([[-3.2, -0.1, -1.3], [0.25, -7.5, 0.7]], np.float32)
        # the product with the centerness spreads the scores: the gap rule holds for sigmoid(cls) alone, so it is asserted on the reference (margin)
        w, m = _check_fcos(be, f'{be.name} fcos level case {ci}', ho, valid0, vs, no, scale, ncls, R, level, pre(n))
        worst, margin = max(worst, w), min(margin, m)
    return worst, margin


# ------------------------------------------------------------------------------------------------------------------ multi-class NMS
def mc_cases():
    """(name, boxes [n, 5], scores [n, stride], num_classes, score_thr, nms_thr, rotated, max_num or None for both sides of the cut)"""
    out = []
    i = 0
    for ncls in (1, 2, 3, 64):
        for n in (1, 64, 65, 200):
            for rotated in (0, 1):
                r = np.random.RandomState(700 + i)
                stride = ncls + (i % 2)                       # score_stride = num_classes + 1 on every other case
                # scores: a grid (gaps >> fp32) permuted; a class with no candidate (all below thr), a class with one, equal scores in two classes
                sc = r.permutation(0.02 + 0.9 * np.arange(n * stride) / (n * stride)).reshape(n, stride).astype(np.float32)
                thr, eq = (0.5, 0.75) if ncls < 64 else (0.9, 0.9625)
                if ncls >= 2:
                    sc[:, 1] = np.minimum(sc[:, 1], 0.3)    # class 1: no candidate
                if ncls >= 3:
                    sc[:, 2] = np.minimum(sc[:, 2], 0.3)
                    sc[n // 2, 2] = 0.97                       # class 2: exactly one
                    sc[0, 0] = sc[n - 1, ncls - 1] = eq        # equal scores in different classes
                sc[n // 3, 0] = thr                            # exactly at the threshold: not a candidate
                boxes = robust(lambda t: _rand_boxes(np.random.RandomState(7000 + i + 1009 * t), n, 0.5 + 1.2 * np.sqrt(n)),
                               lambda bx: multiclass_nms(bx, sc, ncls, thr, 0.25, bool(rotated), 1 << 30)[2], f'mc case {i}')
                out.append((f'mc ncls{ncls} n{n} rot{rotated} stride{stride}', boxes, sc, ncls, thr, 0.25, rotated))
                i += 1
    return out


def run_multiclass(be):
    L, smallest, cut_ties = be.L, np.inf, 0
    for name, boxes, sc, ncls, thr, nms_thr, rotated in mc_cases():
        n, stride = sc.shape
        idx_all, lab_all, margin = multiclass_nms(boxes, sc, ncls, thr, nms_thr, bool(rotated), 1 << 30)
        assert margin >= IOU_MARGIN, f'{name}: the reference decides at |IoU - thr| = {margin:.2e}; choose another seed'
        smallest = min(smallest, margin)
        total = idx_all.size
        s_all = sc[idx_all, lab_all]
        o = np.lexsort((np.arange(total), -s_all.astype(np.float64)))
        between = [p + 1 for p in range(total - 1) if s_all[o[p]] == s_all[o[p + 1]] and lab_all[o[p]] != lab_all[o[p + 1]]]      # a cut between equal scores
        cut_ties += len(between)
        for M in sorted({1, max(total - 1, 1), max(total // 2, 1), total + 2} | set(between)):
            idx, lab, _ = multiclass_nms(boxes, sc, ncls, thr, nms_thr, bool(rotated), M)
            raw, ws, nb = _ws(be, L.ivx_multiclass_nms_workspace_bytes(n, ncls), 'ivx_multiclass_nms_workspace_bytes')
            db, ds = be.up(boxes), be.up(sc)
            oi, ol, oc = be.full((max(M, 1),), np.int64, -7), be.full((max(M, 1),), np.int64, -7), be.full((1,), np.int32, -7)
            be.ok(L.ivx_multiclass_nms_bev(be.ptr(db), be.ptr(ds), n, stride, ncls, thr, nms_thr, rotated, M, ws, nb, be.ptr(oi), be.ptr(ol), be.ptr(oc),
                                           be.stream), 'ivx_multiclass_nms_bev')
            cnt = int(be.get(oc)[0])
            tag = f'{be.name} {name} max_num {M}'
            assert cnt == idx.size, f'{tag}: count {cnt}, expected {idx.size}'
            check_same(tag + ' indices', be.get(oi)[:cnt], idx)
            check_same(tag + ' labels', be.get(ol)[:cnt], lab)
    assert cut_ties >= 1, 'no case cut between equal scores of two classes'
    return smallest


# ------------------------------------------------------------------------------------------------------------------ aligned 3-D NMS
def _boxes6(r, n, spread):
    c = r.uniform(-spread, spread, (n, 3))
    s = r.uniform(0.4, 2.0, (n, 3))
    return np.concatenate([c - s / 2, c + s / 2], 1).astype(np.float32)


def aligned_cases():
    """(name, boxes [n, 6], scores [n], classes [n] int64, thresh)"""
    out = []
    for n in (1, 2, 64, 65, 300):
        def build(t, degenerate):
            r = np.random.RandomState(900 + n + 1009 * t)
            b = _boxes6(r, n, 0.8 + 0.01 * n)
            s = r.permutation(0.05 + 0.9 * np.arange(n) / n).astype(np.float32)
            cl = r.choice(np.array([-3, 0, 1, 64, 70, 1 << 40], np.int64), n)       # negative ids, ids of 64 and above
            if n >= 64:
                s[7] = s[40] = s[41]                                               # bit-equal scores: the lower index first
                b[10] = b[11] = b[12]                                              # identical boxes, one class (10, 11) and another (12)
                cl[10] = cl[11] = 1
                cl[12] = 64
                b[20] = (0, 0, 0, 1, 1, 1)                                         # touching boxes: the intersection has no volume
                b[21] = (1, 0, 0, 2, 1, 1)
                cl[20] = cl[21] = 0
            if degenerate:
                b[30] = b[31] = (0.5, 0.5, 0.5, 0.5, 0.5, 0.5)                     # two zero-volume boxes of different classes: 0 / 0 removes across classes
                cl[30], cl[31] = 0, 1
                b[33, 4] = np.nan                                                  # a NaN corner: NaN volume, removes (and is removed) across classes
            return b, s, cl
        for deg in ((False, True) if n >= 64 else (False,)):
            b, s, cl = robust(lambda t: build(t, deg), lambda x: aligned_3d_nms(x[0], x[1], x[2], 0.25)[1], f'aligned n{n}')
            out.append((f'aligned n{n}' + (' degenerate' if deg else ''), b, s, cl, 0.25))
    return out


def run_aligned(be):
    L, smallest = be.L, np.inf
    for name, b, s, cl, thr in aligned_cases():
        n = b.shape[0]
        pick_ref, margin = aligned_3d_nms(b, s, cl, thr)
        assert margin >= IOU_MARGIN, f'{name}: the reference decides at |IoU - thr| = {margin:.2e}; choose another seed'
        smallest = min(smallest, margin)
        if 'degenerate' in name:
            assert not (31 in pick_ref and 30 in pick_ref), 'the second zero-volume box falls to the first, across classes'
        db, ds, dc = be.up(b), be.up(s), be.up(cl)
        for form in ('plain', 'ws'):
            pick, num = be.full((n,), np.int64, -7), be.full((1,), np.int32, -7)
            if form == 'plain':
                be.ok(L.ivx_aligned_3d_nms(be.ptr(db), be.ptr(ds), be.ptr(dc), n, thr, be.ptr(pick), be.ptr(num), be.stream), 'ivx_aligned_3d_nms')
            else:
                raw, ws, nb = _ws(be, L.ivx_aligned_3d_nms_workspace_bytes(n), 'ivx_aligned_3d_nms_workspace_bytes')
                be.ok(L.ivx_aligned_3d_nms_ws(be.ptr(db), be.ptr(ds), be.ptr(dc), n, thr, ws, nb, be.ptr(pick), be.ptr(num), be.stream),
                      'ivx_aligned_3d_nms_ws')
            k = int(be.get(num)[0])
            tag = f'{be.name} {name} ({form})'
            assert k == pick_ref.size, f'{tag}: {k} picks, expected {pick_ref.size}'
            check_same(tag, be.get(pick)[:k], pick_ref)
    return smallest


# ------------------------------------------------------------------------------------------------------------------ indoor tails
def indoor_cases():
    """(name, R, ks, ncls, score_thr, nms_thr, rotated, max_sel, special)"""
    out = []
    for li, ks in enumerate([(37,), (40, 23, 9), (33, 64, 5, 17)]):
        out.append((f'scannet L{len(ks)}', 6, ks, (18, 3, 2)[li], 0.3, 0.25, 0, 'all', 'at_thr'))
        out.append((f'scannet L{len(ks)} cut', 6, ks, 2, 0.3, 0.25, 0, 'fewer', 'label_tie'))
    out.append(('scannet all below', 6, (12, 7), 3, 0.99, 0.25, 0, 'all', None))
    for li, ncls in enumerate((1, 2, 3, 10)):
        ks = [(37,), (40, 23, 9), (33, 64, 5, 17), (20, 11, 3)][li]
        out.append((f'sunrgbd ncls{ncls} L{len(ks)}', 7, ks, ncls, 0.3, 0.25, li % 2, ('all', 'fewer')[li % 2], None))
    return out


def run_indoor(be):
    L, worst, smallest = be.L, 0.0, np.inf
    for ci, (name, R, ks, ncls, sthr, nthr, rotated, max_sel, special) in enumerate(indoor_cases()):
        B, K = 2, sum(ks)

        def build(t):
            r = np.random.RandomState(1200 + ci + 1009 * t)
            if R == 6:
                boxes = np.stack([_boxes6(r, K, 1.2) for _ in range(B)])
            else:
                c, s = r.uniform(-1, 1, (B, K, 3)) * (0.5 + 0.5 * np.sqrt(K)), r.uniform(0.4, 2.0, (B, K, 3))
                boxes = np.concatenate([c, s, r.uniform(-np.pi, np.pi, (B, K, 1))], 2).astype(np.float32)
            sc = np.stack([r.permutation(0.02 + 0.9 * np.arange(K * ncls) / (K * ncls)).reshape(K, ncls) for _ in range(B)]).astype(np.float32)
            if special == 'at_thr':
                j = int(np.argmax(sc[0].max(1) < sthr)) if (sc[0].max(1) < sthr).any() else 0
                sc[0, j, :] = np.minimum(sc[0, j, :], np.float32(sthr))
                sc[0, j, ncls - 1] = sthr                                            # the best score equals score_thr: not a candidate
            if special == 'label_tie':
                sc[:, 3, :] = 0.8125                                                 # two classes with the same maximum: the first
            one = (lambda b, M: indoor_tail_scannet(boxes[b], sc[b], sthr, nthr, M)) if R == 6 else \
                (lambda b, M: indoor_tail_sunrgbd(boxes[b], sc[b], sthr, nthr, bool(rotated), M))
            refs = [one(b, 1 << 30) for b in range(B)]
            M = K * ncls if max_sel == 'all' else max(len(refs[0][2]) - 2, 1)
            if max_sel == 'fewer':
                refs = [one(b, M) for b in range(B)]
            return boxes, sc, M, refs
        boxes, sc, M, refs = robust(build, lambda x: min(rf[4] for rf in x[3]), f'indoor {name}')
        desc = be.IndoorTailDesc(B=B, n_levels=len(ks), k=(C.c_int32 * 4)(*(list(ks) + [0] * (4 - len(ks)))), n_classes=ncls, n_reg=R, use_rotate_nms=rotated,
                              max_num=M, score_thr=sthr, nms_thr=nthr)
        raw, ws, nb = _ws(be, L.ivx_indoor_tail_workspace_bytes(C.byref(desc)), 'ivx_indoor_tail_workspace_bytes')
        offs = np.concatenate([[0], np.cumsum(ks)])
        lb = [be.up(boxes[:, offs[l]:offs[l + 1]]) for l in range(len(ks))]
        ls = [be.up(sc[:, offs[l]:offs[l + 1]]) for l in range(len(ks))]
        pb = (C.c_void_p * 4)(*([be.ptr(t) for t in lb] + [None] * (4 - len(ks))))
        ps = (C.c_void_p * 4)(*([be.ptr(t) for t in ls] + [None] * (4 - len(ks))))
        ob, os_, ol, oc = be.full((B, M, 7), np.float32, np.nan), be.full((B, M), np.float32, np.nan), be.full((B, M), np.int64, -7), be.full((B,), np.int32, -7)
        be.ok(L.ivx_indoor_tail_get_bboxes(C.byref(desc), pb, ps, ws, nb, be.ptr(ob), be.ptr(os_), be.ptr(ol), be.ptr(oc), be.stream),
              'ivx_indoor_tail_get_bboxes')
        ob, os_, ol, oc = (be.get(t) for t in (ob, os_, ol, oc))
        for b, (rows, bound, rs, rl, margin) in enumerate(refs):
            tag = f'{be.name} indoor {name} sample {b}'
            assert margin >= IOU_MARGIN, f'{tag}: the reference decides at |IoU - thr| = {margin:.2e}; choose another seed'
            smallest = min(smallest, margin)
            cnt = len(rs)
            assert int(oc[b]) == cnt, f'{tag}: count {int(oc[b])}, expected {cnt}'
            if name == 'scannet all below':
                assert cnt == 0
            check_same(tag + ' labels', ol[b, :cnt], rl)
            check_same(tag + ' scores (copies)', os_[b, :cnt], rs.astype(np.float32))
            worst = max(worst, check_close(tag + ' rows', ob[b, :cnt], rows, bound))
            assert not ob[b, cnt:].any() and not os_[b, cnt:].any() and not ol[b, cnt:].any(), tag + ': rows beyond count must be zero'
    return worst, smallest
