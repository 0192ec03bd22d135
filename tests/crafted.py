"""Crafted plane fields for the kernels that shape their work from the field they are handed -- pm::sweep_group_kernel /
pm::group_kernel (pm_group.h), pm::push_kernel (pm_push.h) -- and a plain CPU census of what the first launch after such a
field is installed has to do, tile by tile ("crafted fields").  No GPU is needed for anything in here.

Conventions restated from the kernels (pm_sweep.h): black <=> (x + y) even; tiles of 32 x 16 pixels with an even origin;
candidate slot k of a pixel = its neighbour up, down, left, right at distance 1 (k = 0..3) and 5 (k = 4..7), offered only
inside the frame; a slot is a TASK unless its plane equals, bit for bit, the pixel's own (rule (A)) or that of an earlier
offered slot (rule (D)); tasks with the same plane bits and the same x parity of the owner form a GROUP, whose samples
fill the bounding box of its owners' windows: N + dx / 2 strips of N + dy / 2 rows, N = (box + 1) / 2."""
import ctypes as C

import numpy as np

TILE_W, TILE_H = 32, 16
HASH_SIZE = 2048                      # pm::kGrpHashSize
MAX_TASKS = 2048                      # pm::kGrpMaxTasks = 8 slots x 256 pixels of a colour
BATCH_GROUPS, BATCH_STRIPS, BATCH_TASKS = 8, 64, 64
SLOTS = [(0, -1), (0, 1), (-1, 0), (1, 0), (0, -5), (0, 5), (-5, 0), (5, 0)]  # (dx, dy) of slot k

FIELDS = ["one", "interleaved-3", "interleaved-8", "interleaved-40", "blocks-2x2", "blocks-4x4", "blocks-8x4", "blocks-16x8",
          "distinct", "nothing", "collide-12", "degenerate", "degenerate-nan"]
COLLIDE_RAW = 2043                    # raw hash of the colliding planes: chains of both classes cross slot 2047 -> 0


def batch_samples(box):
    return 1280 if box == 25 else 1024    # pm::group_batch_samples


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def plane_hash(planes, cls=0):
    """pm::plane_hash on an array of planes (..., 4): uint32 arithmetic with wrap-around"""
    b = bits(planes).astype(np.uint64)
    m = np.uint64(0xFFFFFFFF)
    h = (b[..., 0] * np.uint64(0x9E3779B1)) & m
    h = ((h ^ b[..., 1]) * np.uint64(0x85EBCA77)) & m
    h = ((h ^ b[..., 2]) * np.uint64(0xC2B2AE3D)) & m
    h = ((h ^ b[..., 3]) * np.uint64(0x27D4EB2F)) & m
    h ^= h >> np.uint64(15)
    return ((h + np.uint64(cls)) & np.uint64(HASH_SIZE - 1)).astype(np.int64)


def _ref_cam(gs):
    cam = gs.cameras.c_array[0]
    return np.float32(cam.fx), np.float32(cam.K[2]), np.float32(cam.K[5])


def plane_at(gs, n, depth, x, y):
    """the plane with normal n that has `depth` at pixel (x, y): d = -n.X, as tests.test_parity_gpu.random_planes forms it"""
    fx, cx, cy = _ref_cam(gs)
    n = np.asarray(n, dtype=np.float32)
    n = n / np.float32(np.linalg.norm(n))
    X = np.array([(np.float32(x) - cx) / fx * depth, (np.float32(y) - cy) / fx * depth, depth], dtype=np.float32)
    return np.array([n[0], n[1], n[2], -(n * X).sum(dtype=np.float32)], dtype=np.float32)


def pool(gs, m, seed):
    """m distinct, gently tilted planes that are plausible over the whole frame"""
    rng = np.random.default_rng(seed)
    out = np.empty((m, 4), dtype=np.float32)
    for i in range(m):
        n = np.array([rng.uniform(-0.15, 0.15), rng.uniform(-0.15, 0.15), -1.0])
        depth = np.float32(rng.uniform(gs.params.depthMin * 1.3, gs.params.depthMax * 0.7))
        out[i] = plane_at(gs, n, depth, gs.cols // 2, gs.rows // 2)
    assert len({p.tobytes() for p in out}) == m
    return out


def colliding_planes(gs, k, seed, raw=COLLIDE_RAW):
    """k distinct planes with one plane_hash (and so one hash slot per class): a pool plane whose w is stepped ulp by ulp"""
    q = pool(gs, 1, seed)[0]
    cand = np.tile(q, (1 << 17, 1))
    w = bits(cand[:, 3].copy()) + np.arange(1 << 17, dtype=np.uint32)
    cand[:, 3] = w.view(np.float32)
    hit = cand[plane_hash(cand) == raw][:k]
    assert len(hit) == k, "search space too small"
    return hit


def random_planes(gs, seed):
    from tests.test_parity_gpu import random_planes as rp
    return rp(gs, seed=seed)


def degenerate_pool(gs, seed, with_nan):
    """planes a whole group shares so that its strips take the guarded paths; returns (planes, kinds)"""
    good = pool(gs, 6, seed)
    kinds, pl = [], []

    def add(kind, p):
        kinds.append(kind)
        pl.append(np.asarray(p, dtype=np.float32))
    add("plain", good[0])
    add("d-zero", good[1] * np.float32([1, 1, 1, 0]))             # homography divides by d: infinite entries, no safe window
    add("d-tiny", good[2] * np.float32([1, 1, 1, 1e-30]))         # entries beyond 2^40
    add("d-small", good[2] * np.float32([1, 1, 1, 1e-3]))         # a surface 0.5 mm in front of the camera
    add("behind", good[3] * np.float32([1, 1, 1, -1]))            # negative depth
    add("too-far", good[4] * np.float32([1, 1, 1, 3]))            # depth beyond depthMax
    add("too-near", good[4] * np.float32([1, 1, 1, 0.3]))         # depth under depthMin
    z = plane_at(gs, [0.0, 0.1, -1.0], np.float32(0.5 * (gs.params.depthMin + gs.params.depthMax)), gs.cols // 2, gs.rows // 2)
    zp, zn = z.copy(), z.copy()
    zp[0], zn[0] = np.float32(0.0), np.float32(-0.0)
    add("zero+", zp)                                              # equal as numbers, different as bits: two groups
    add("zero-", zn)
    if with_nan:
        add("nan", good[5] * np.float32([1, 1, 1, np.nan]))
    return np.stack(pl), kinds


def make_field(name, gs, colour=0, seed=7):
    """(rows, cols, 4) planes: the pixels of `colour` (swept by the first launch) keep plausible distinct planes, the
    pixels of the other colour -- the sources of that launch's candidates -- hold the crafted pattern"""
    rows, cols = gs.rows, gs.cols
    base = random_planes(gs, seed)
    ys, xs = np.mgrid[0:rows, 0:cols]
    other = ((xs + ys) & 1) != colour
    f = base.copy()
    if name == "distinct":
        return f
    if name == "one":
        f[other] = pool(gs, 1, seed + 1)[0]
    elif name == "nothing":
        f[:] = pool(gs, 1, seed + 1)[0]
    elif name.startswith("interleaved-"):
        m = int(name.split("-")[1])
        q = pool(gs, m, seed + 2)
        idx = ((xs >> 1) * 7 + ys * 11) % m
        f[other] = q[idx[other]]
    elif name.startswith("blocks-"):
        w, h = (int(v) for v in name.split("-")[1].split("x"))
        alt = random_planes(gs, seed + 3)
        # block grid shifted by half a block: blocks straddle the tile borders at multiples of 32 / 16
        ax = np.clip(((xs + w // 2) // w) * w - w // 2, 0, cols - 1)
        ay = np.clip(((ys + h // 2) // h) * h - h // 2, 0, rows - 1)
        f[other] = alt[ay, ax][other]
    elif name.startswith("collide-"):
        k = int(name.split("-")[1])
        q = colliding_planes(gs, k, seed + 4)
        idx = ((xs >> 1) * 5 + ys * 3) % (2 * k)
        idx = np.where(idx < k, idx, 0)       # half of the sources hold q[0]: the `one` share, matches inside the chain
        f[other] = q[idx[other]]
    elif name in ("degenerate", "degenerate-nan"):
        q, _ = degenerate_pool(gs, seed + 5, name.endswith("nan"))
        idx = (((xs + 2) // 4) + 3 * ((ys + 2) // 4)) % len(q)   # 4x4 blocks, shifted
        f[other] = q[idx[other]]
    else:
        raise ValueError(name)
    return np.ascontiguousarray(f, dtype=np.float32)


def census(planes, colour, box=15):
    """What the first launch of `colour` after the install has to do, per 32 x 16 tile (row-major list of dicts):
    n_pixels, n_tasks, groups = [(tasks, strips, rows, plane bytes, parity)], probe = the longest linear-probing walk of
    the 2048-slot table when the groups are inserted, wrapped = a walk stepped from slot 2047 to slot 0"""
    rows, cols = planes.shape[:2]
    n_half = (box + 1) // 2
    key = [[bits(planes[y, x]).tobytes() for x in range(cols)] for y in range(rows)]
    tiles = []
    for y0 in range(0, rows, TILE_H):
        for x0 in range(0, cols, TILE_W):
            groups = {}
            n_tasks = n_pix = 0
            for y in range(y0, min(y0 + TILE_H, rows)):
                for x in range(x0 + ((y + colour) & 1), min(x0 + TILE_W, cols), 2):
                    n_pix += 1
                    seen = [key[y][x]]
                    for dx, dy in SLOTS:
                        xx, yy = x + dx, y + dy
                        if not (0 <= xx < cols and 0 <= yy < rows):
                            continue
                        k = key[yy][xx]
                        if k in seen:
                            continue
                        seen.append(k)
                        n_tasks += 1
                        g = groups.setdefault((k, x & 1), [0, x, x, y, y])
                        g[0] += 1
                        g[1], g[2], g[3], g[4] = min(g[1], x), max(g[2], x), min(g[3], y), max(g[4], y)
            glist = [(g[0], n_half + (g[2] - g[1]) // 2, n_half + (g[4] - g[3]) // 2, k, par) for (k, par), g in groups.items()]
            # linear probing: which slots end up occupied does not depend on the insertion order, nor does whether the
            # boundary 2047 -> 0 is crossed; the longest walk of THIS order is a lower bound of the kernel's worst order
            table, probe, wrapped = set(), 0, False
            for (_, _, _, k, par) in sorted(glist, key=lambda g: (g[3], g[4])):
                h = int(plane_hash(np.frombuffer(k, dtype=np.float32), par))
                steps = 0
                while h in table:
                    if h == HASH_SIZE - 1:
                        wrapped = True
                    h = (h + 1) & (HASH_SIZE - 1)
                    steps += 1
                table.add(h)
                probe = max(probe, steps)
            tiles.append(dict(x0=x0, y0=y0, n_pixels=n_pix, n_tasks=n_tasks, groups=glist, probe=probe, wrapped=wrapped))
    return tiles


def batch_replay(groups, box):
    """The two-ended batch cursor of pm_group.h (group_costs, "take the next batch") replayed for one tile by ONE consumer:
    the groups ordered by row count (the counting sort; ties in list order -- the kernel's tie order is whatever its atomics
    give, and with four wavefronts the batches interleave, so this is one of the possible histories), a batch filled from
    the long-strip end while strips <= 64, tasks <= 64 and strips x (rows | 1) <= the sample buffer, at most 8 groups, then
    from the short-strip end under the same sums.  Returns one dict per batch: groups, strips, tasks, rows, and `top` /
    `bottom` = what stopped that fill: 'end' (no group left), 'groups' (the 8-group limit), 'rounds' (a single group of
    more than 64 tasks: it is taken alone and chained in several rounds), or the limits the refused group would have broken
    joined by '+', from 'strips', 'tasks', 'samples'."""
    n_half = (box + 1) // 2
    cap = batch_samples(box)
    order = sorted(groups, key=lambda g: (g[2] - n_half) & 7)   # ascending; the top of the order is its end
    lo, hi, n = 0, 0, len(order)
    out = []

    def broken(strips, tasks, nrs):
        b = []
        if strips > BATCH_STRIPS:
            b.append("strips")
        if tasks > BATCH_TASKS:
            b.append("tasks")
        if strips * nrs > cap:
            b.append("samples")
        return "+".join(b)

    while n - lo - hi > 0:
        remaining = n - lo - hi
        nrs = order[n - 1 - hi][2] | 1
        strips = tasks = k1 = 0
        top = "end"
        for rank in range(min(BATCH_GROUPS, remaining)):
            g = order[n - 1 - hi - rank]
            why = broken(strips + g[1], tasks + g[0], nrs)
            if why:
                top = why
                break
            strips, tasks, k1 = strips + g[1], tasks + g[0], k1 + 1
        else:
            if remaining > BATCH_GROUPS:
                top = "groups"
        if k1 == 0:  # a single group always fits the strips and the buffer; more than 64 tasks: several rounds
            g = order[n - 1 - hi]
            assert g[1] <= BATCH_STRIPS and g[1] * nrs <= cap and g[0] > BATCH_TASKS
            strips, tasks, k1, top = g[1], g[0], 1, "rounds"
        k2 = 0
        bottom = "end"
        for rank in range(BATCH_GROUPS):
            if rank >= remaining - k1:
                break
            if rank >= BATCH_GROUPS - k1:
                bottom = "groups"
                break
            g = order[lo + rank]
            why = broken(strips + g[1], tasks + g[0], nrs)
            if why:
                bottom = why
                break
            strips, tasks, k2 = strips + g[1], tasks + g[0], k2 + 1
        out.append(dict(groups=k1 + k2, from_bottom=k2, strips=strips, tasks=tasks, rows=order[n - 1 - hi][2],
                        top=top, bottom=bottom))
        hi += k1
        lo += k2
    return out


def batch_stops(tiles, box):
    """how often each stop reason occurs over all fills (top and bottom) of all batches of all tiles (batch_replay)"""
    from collections import Counter
    c = Counter()
    for t in tiles:
        for b in batch_replay(t["groups"], box):
            c[b["top"]] += 1
            c[b["bottom"]] += 1
            if b["from_bottom"]:
                c["mixed-ends"] += 1
            if b["tasks"] <= 32:
                c["tasks<=32"] += 1
            elif b["tasks"] <= 64:
                c["tasks33-64"] += 1
    return c


def summary(tiles, box=15):
    """the figures DESIGN.md 4 quotes per case: maxima over the tiles, and the batch stops of batch_replay"""
    full_strips, full_rows = (box + 1) // 2 + (TILE_W - 1) // 2, (box + 1) // 2 + (TILE_H - 1) // 2
    return dict(
        tiles=len(tiles),
        max_tasks=max(t["n_tasks"] for t in tiles), min_tasks=min(t["n_tasks"] for t in tiles),
        max_groups=max(len(t["groups"]) for t in tiles),
        max_group_tasks=max([g[0] for t in tiles for g in t["groups"]] or [0]),
        full_tile_groups=max(sum(1 for g in t["groups"] if g[1] == full_strips and g[2] == full_rows) for t in tiles),
        strip_lengths=sorted({g[2] for t in tiles for g in t["groups"]}),
        probe=max(t["probe"] for t in tiles), wrapped=any(t["wrapped"] for t in tiles),
        stops=batch_stops(tiles, box))


def unsafe_views(gs, plane, x0, x1, y0, y1):
    """views in which pm::window_div_safe must refuse the box [x0, x1] x [y0, y1] for `plane`, judged from the oracle's
    homography with wide margins (a non-finite entry; |H2| or |H5| under 2^-37; a corner Z beyond 2^41, under 2^-41 or of
    another sign than the other corners) -- a subset of the kernel's own refusals that no rounding can move"""
    from tests import oracle_lib
    L = oracle_lib.lib()
    out = []
    pl = np.ascontiguousarray(plane, dtype=np.float32)
    for v in range(gs.desc.n_selected):
        H = np.zeros(9, dtype=np.float32)
        L.gipuma_oracle_homography(C.byref(gs.cameras.c_array[0]), C.byref(gs.cameras.c_array[gs.desc.selected[v]]),
                                   oracle_lib.fptr(pl), float(pl[3]), oracle_lib.fptr(H))
        H = H.astype(np.float64)
        bad = not np.isfinite(H).all() or abs(H[2]) < 2.0 ** -37 or abs(H[5]) < 2.0 ** -37
        if not bad:
            z = np.array([H[6] * qx + H[7] * qy + H[8] for qx in (x0, x1) for qy in (y0, y1)])
            bad = bool((np.abs(z) > 2.0 ** 41).any() or (np.abs(z) < 2.0 ** -41).any() or (z.min() < 0 < z.max()))
        if bad:
            out.append(v)
    return out
