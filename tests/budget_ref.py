"""numpy twin of "WATER BUDGET" in include/suhmo_hip.h: tests/massbalance_ref.py's seven terms, the volume-only reduction a tracked time step
leaves on the device (k_volume) and the two recharge terms (wb_cell of suhmo_amd/csrc/suhmo_balance.h, which restates d_postproc_columns per cell),
summed in the first_stage_seq / second-stage order of tests/reduce_ref.py: change one, change the other.  One array statement per statement of
the rule, so that the device is compared bit for bit.

recharge       ice = mask > 0;  src = use_moulin_source ? MSRC * ramp + distributed_input : (ice ? distributed_input : 0.0)
               ice:  ext += src * dy * dx;  melt += (MR / rho_w) * dy * dx  -- after the cell's volume term, each into its own accumulator; a
               term that is not there is +0.0 (massbalance_ref: no bit of a sum that started from +0.0 changes)
volume_old     the VOLUME reduction alone, over the mask and gap height the step started from: one value per workgroup on the same grid, the same
               second stage -- by construction the bits of VOLUME of massbalance_ref.level_balance on the same data"""
import numpy as np

from tests import massbalance_ref as mb
from tests import reduce_ref as rr

NAMES = mb.NAMES + ("volume_old", "recharge_ext", "recharge_melt")
VOLUME_OLD, RECH_EXT, RECH_MELT = 7, 8, 9
# where the nine sums of a first stage go in the row of ten
FROM_SUMS = tuple(range(7)) + (RECH_EXT, RECH_MELT)


def recharge_terms(mask_g, mr, msrc, dx, dy, mp):
    """-> (ext, melt): the (ny, nx) arrays the thread of a cell adds; msrc: the source term (valid cells) where mp["use_moulin_source"], else unused"""
    m = np.asarray(mask_g, dtype=np.float64)[1:-1, 1:-1]
    ice = m > 0.0
    with np.errstate(over="ignore", invalid="ignore"):
        if mp["use_moulin_source"]:
            src = np.asarray(msrc, dtype=np.float64) * mp["ramp"] + mp["distributed_input"]
        else:
            src = np.where(ice, mp["distributed_input"], 0.0)
        ext = np.where(ice, src * dy * dx, 0.0)
        melt = np.where(ice, (np.asarray(mr, dtype=np.float64) / mp["rho_w"]) * dy * dx, 0.0)
    return ext, melt


def terms_of(d, box, domain, bc, dx, dy, mp):
    """d: massbalance_ref's data of a box plus mr= and msrc= (valid cells; msrc may be None without a moulin source) -> seq[0 .. 8]"""
    seq = mb.terms_of(d, box, domain, bc, dx, dy)
    ext, melt = recharge_terms(d["mask"], d["mr"], d.get("msrc"), dx, dy, mp)
    return seq + [[ext], [melt]]


def reduce_level(boxes_seq, q, cap):
    """value q of a level: the first stage of every box on the grid of the level's largest box extents, boxes ascending, then the second stage"""
    my = max(s[mb.VOLUME][0].shape[0] for s in boxes_seq)
    mx = max(s[mb.VOLUME][0].shape[1] for s in boxes_seq)
    return rr.second_stage(np.concatenate([mb.first_stage_seq(s[q], (my, mx), cap) for s in boxes_seq]))


def volume_only(boxes_seq, cap):
    """k_volume and the final stage's walk over its partials: VOLUME alone (boxes_seq: terms_of, or massbalance_ref.terms_of, of every box)"""
    return reduce_level(boxes_seq, mb.VOLUME, cap)


def level_budget(boxes_seq, cap, volume_old=np.nan):
    """boxes_seq[k]: terms_of of box k -> (10,); volume_old: what volume_only gave on the state the step started from (NaN: no tracked step)"""
    out = np.full(len(NAMES), np.nan)
    for q, where in enumerate(FROM_SUMS):
        out[where] = reduce_level(boxes_seq, q, cap)
    out[VOLUME_OLD] = volume_old
    return out


def default_cap(boxes, domain):
    return rr.CAP_LEVEL if len(boxes) == 1 and tuple(boxes[0]) == (0, 0, domain[0] - 1, domain[1] - 1) else rr.CAP_BOX


def budget_of_level(data, boxes, domain, bc, dx, dy, mp, cap=None, volume_old=np.nan):
    cap = cap if cap is not None else default_cap(boxes, domain)
    return level_budget([terms_of(d, b, domain, bc, dx, dy, mp) for d, b in zip(data, boxes)], cap, volume_old)


def volume_of_level(data, boxes, domain, bc, dx, dy, cap=None):
    cap = cap if cap is not None else default_cap(boxes, domain)
    return volume_only([mb.terms_of(d, b, domain, bc, dx, dy) for d, b in zip(data, boxes)], cap)


def volume_of_boxes(masks_g, Bs, dx, dy, cap):
    """the same from what k_volume reads alone: the ghosted mask and the gap height (valid cells, or ghosted) of every box of a level"""
    seqs = []
    for m, B in zip(masks_g, Bs):
        m = np.asarray(m, dtype=np.float64)[1:-1, 1:-1]
        B = B if B.shape == m.shape else B[1:-1, 1:-1]
        s = [None] * len(mb.NAMES)
        with np.errstate(over="ignore", invalid="ignore"):
            s[mb.VOLUME] = [np.where(m > 0.0, B * dx * dy, 0.0)]
        seqs.append(s)
    return volume_only(seqs, cap)


def synthetic_recharge(nx, ny, seed):
    """melt rate and source term over a level's valid cells for the tests that need no device: multiples of 2^-20 of magnitude 1 .. 4"""
    rng = np.random.default_rng([int(seed), 4099, nx, ny])
    q = lambda shape: np.round(rng.uniform(1.0, 4.0, size=shape) * 2.0 ** 20) / 2.0 ** 20
    return q((ny, nx)), q((ny, nx))


def cut_valid(a, box):
    """the valid cells of a box out of a level's (ny, nx) array"""
    lo0, lo1, hi0, hi1 = box
    return np.ascontiguousarray(a[lo1:hi1 + 1, lo0:hi0 + 1])
