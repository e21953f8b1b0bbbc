"""Float64 numpy restatements of FABind+'s confidence bookkeeping, the references of tests/test_ranking_refs_cpu.py and
tests/test_gpu_ranking.py.  Each function restates the cited lines of the reference tree (FABind_plus/fabind/) as they are written:
the literal double loop, not a vectorised equivalent."""
import numpy as np


def _sigmoid(x):
    e = np.exp(-abs(x))
    return 1.0 / (1.0 + e) if x >= 0 else e / (1.0 + e)


def pose_stats_ref(pred, truth, atom_off):
    """utils/training_confidence.py:41-46: rmsd = sqrt(scatter_mean(|p - t|^2)), centroid distance = |scatter_mean(p) -
    scatter_mean(t)|; an empty sample gives 0 (scatter_mean's empty row).  -> (rmsd [B], cdis [B], max_i |p_i - t_i| [B])."""
    p, t = np.asarray(pred, dtype=np.float64), np.asarray(truth, dtype=np.float64)
    B = len(atom_off) - 1
    rmsd, cdis, dmax = np.zeros(B), np.zeros(B), np.zeros(B)
    for b in range(B):
        lo, hi = int(atom_off[b]), int(atom_off[b + 1])
        if hi <= lo:
            continue
        d = p[lo:hi] - t[lo:hi]
        rmsd[b] = np.sqrt((d ** 2).sum(-1).mean())
        cdis[b] = np.linalg.norm(p[lo:hi].mean(0) - t[lo:hi].mean(0))
        dmax[b] = np.sqrt((d ** 2).sum(-1)).max()
    return rmsd, cdis, dmax


def stable_order(rmsd):
    """rmsd.argsort() (:50) made stable: ascending (rmsd, index).  The reference's order on an exact tie is unspecified."""
    return sorted(range(len(rmsd)), key=lambda a: (rmsd[a], a))


def rank_group_ref(scores, rmsd, mode="logsigmoid", with_ce=False):
    """utils/training_confidence.py:48-77 for one group (the reference's whole batch).  -> dict: ranking, ce, loss, grad
    (d loss / d scores, relu' = 0 at 0), counts (ranked_right, pairs, hit, confidence_correct), mean_abs_term (the mean |pair term|)
    and mean_abs_ce (the mean |BCE term|, 0 without it)."""
    s, r = np.asarray(scores, dtype=np.float64), np.asarray(rmsd, dtype=np.float64)
    S = len(s)
    order = stable_order(r)
    ss, sr = s[order], r[order]                                   # :50-51
    total, abs_total, right = 0.0, 0.0, 0
    gs = np.zeros(S)
    for i in range(S):                                            # :56-65
        for j in range(i):                                        # j is better than i
            d = ss[j] - ss[i]
            if mode == "dynamic_hinge":
                m = (sr[i] - sr[j]) - d
                t, dt = max(m, 0.0), (-1.0 if m > 0 else 0.0)     # F.relu; dt = d t / d d
            elif mode == "logsigmoid":
                t, dt = max(-d, 0.0) + np.log1p(np.exp(-abs(d))), -_sigmoid(-d)   # -F.logsigmoid(d)
            else:
                raise ValueError(mode)
            total += t
            abs_total += abs(t)
            gs[j] += dt
            gs[i] -= dt
            right += int(ss[j] > ss[i])                           # :65
    P = S * (S - 1) / 2
    ranking = total / P                                           # :67
    grad = np.zeros(S)
    grad[order] = gs / P
    y = (r < 2).astype(np.float64)                                # :54
    ce, mean_abs_ce = 0.0, 0.0
    if with_ce:                                                   # :68-70, BCEWithLogitsLoss (mean)
        bce = np.array([max(x, 0.0) - x * yy + np.log1p(np.exp(-abs(x))) for x, yy in zip(s, y)])
        ce, mean_abs_ce = bce.mean(), np.abs(bce).mean()
        grad = grad + np.array([_sigmoid(x) - yy for x, yy in zip(s, y)]) / S
    hit = int(ss[0] > ss[1:].max())                               # :76
    conf = int((float(s[0] > 0) == y).sum())                      # :77 -- the FIRST score against every sample's label
    return dict(ranking=ranking, ce=ce, loss=ranking + ce, grad=grad, counts=np.array([right, int(P), hit, conf]),
                mean_abs_term=abs_total / P, mean_abs_ce=mean_abs_ce)


def rank_ref(scores, rmsd, sizes, mode="logsigmoid", with_ce=False):
    """Consecutive groups of `sizes` samples, each ranked on its own; the loss is the mean over the groups.  -> (dict of the means
    with grad over all samples and counts [G, 4], list of the per-group dicts)."""
    s, r = np.asarray(scores, dtype=np.float64), np.asarray(rmsd, dtype=np.float64)
    assert sum(sizes) == len(s)
    per, o = [], 0
    for n in sizes:
        per.append(rank_group_ref(s[o:o + n], r[o:o + n], mode, with_ce))
        o += n
    G = len(sizes)
    out = {k: sum(p[k] for p in per) / G for k in ("ranking", "ce", "loss")}
    out["grad"] = np.concatenate([p["grad"] for p in per]) / G
    out["counts"] = np.stack([p["counts"] for p in per])
    return out, per


def metrics_ref(batches):
    """utils/training_confidence.py:258-326: the validation dictionary over `batches`, each a dict of what one loop iteration
    sees: scores, rmsd, cdis [B], logits / mask [B, L] (pocket_cls_pred, protein_out_mask_whole), less5, mode, with_ce."""
    rmsd, cdis = [], []
    acc, hit, conf_ok, tot, rk, ce, count, skip, less5 = [], 0.0, 0.0, 0.0, 0.0, 0.0, 0, 0, 0
    for b in batches:
        s, r = np.asarray(b["scores"], dtype=np.float64), np.asarray(b["rmsd"], dtype=np.float64)
        g = rank_group_ref(s, r, b["mode"], b["with_ce"])
        right, P, h, c = [int(v) for v in g["counts"]]
        acc += [1.0] * right + [0.0] * (P - right)               # ranking_accuracy_list (:240)
        hit += h
        conf_ok += c
        tot += len(s) * g["loss"]                                 # :258-260
        rk += len(s) * g["ranking"]
        ce += len(s) * g["ce"]
        less5 += int(b["less5"])
        rmsd.append(r)
        cdis.append(np.asarray(b["cdis"], dtype=np.float64))
        logits, mask = np.asarray(b["logits"], dtype=np.float64), np.asarray(b["mask"]).astype(bool)
        for i, j in enumerate(mask.sum(1)):                       # :272-279
            count += 1
            pred = np.round(1.0 / (1.0 + np.exp(-logits[i][:j]))).astype(int) == 1
            skip += int(pred.sum() == 0)
    rmsd, cdis = np.concatenate(rmsd), np.concatenate(cdis)
    m = {"samples": count, "skip_samples": skip, "keepNode < 5": less5}
    for x, p in ((rmsd, "rmsd"), (cdis, "centroid_dis")):          # :315-318
        m.update({p: x.mean(), p + " < 2A": (x < 2).mean(), p + " < 5A": (x < 5).mean()})
        m.update({p + " 25%": np.quantile(x, 0.25), p + " 50%": np.quantile(x, 0.50), p + " 75%": np.quantile(x, 0.75)})
    n = len(rmsd)
    m.update({"confidence_loss": tot / n, "ranking_loss": rk / n, "confidence_ce_loss": ce / n,       # :320-326
              "confidence_accuracy": conf_ok / n, "ranking_accuracy": sum(acc) / len(acc) if len(acc) > 0 else 0.,
              "hit_rate": hit / n})
    return m


def select_ref(rmsds, cdiss, confs, N=1):
    """test_sampling_fabind.py:159-175: [S, B] arrays -> (min rmsd, min centroid distance) among the N most confident samples."""
    rmsds, cdiss, confs = (np.asarray(v, dtype=np.float64) for v in (rmsds, cdiss, confs))
    choice = confs.argsort(axis=0)[::-1][:N]                     # :163
    tr, tc = [], []
    for i in range(rmsds.shape[1]):                               # :167-175
        tr.append(min(rmsds[choice[j][i]][i] for j in range(N)))
        tc.append(min(cdiss[choice[j][i]][i] for j in range(N)))
    return np.array(tr), np.array(tc)


def sampling_metrics_ref(rmsds, cdiss, confs, N=1):
    """test_sampling_fabind.py:177-191 with the test set's size B in place of the hard-coded 363."""
    r, c = select_ref(rmsds, cdiss, confs, N)
    B = len(r)
    m = {}
    for x, p in ((r, "rmsd"), (c, "centroid_dis")):
        m.update({p + "_mean": np.mean(x), p + "_2A": np.sum(x < 2) / B, p + "_5A": np.sum(x < 5) / B,
                  p + "_25": np.quantile(x, 0.25), p + "_50": np.quantile(x, 0.50), p + "_75": np.quantile(x, 0.75)})
    return m


def make_rank_inputs(sizes, seed):
    """Random scores / rmsds for groups of `sizes`, as float32 arrays: rmsds of a group at least 0.03 A apart and 2e-3 A away from
    the 2 A and 5 A thresholds, scores ~ N(0, 1.5).  The tests assert these conditions on the float64 copy."""
    rng = np.random.default_rng(seed)
    sc, rm = [], []
    for S in sizes:
        step = 7.5 / max(S, 16)
        r = 0.25 + (np.arange(S) + 0.5) * step + rng.uniform(-0.2, 0.2, S) * step
        for thr in (2.0, 5.0):
            near = np.abs(r - thr) < 2e-3
            r[near] = thr + 4e-3
        rm.append(rng.permutation(r))
        sc.append(rng.normal(0.0, 1.5, S))
    return np.concatenate(sc).astype(np.float32), np.concatenate(rm).astype(np.float32)


def assert_rank_input_conditions(scores, rmsd, sizes):
    s, r = np.asarray(scores, dtype=np.float64), np.asarray(rmsd, dtype=np.float64)
    assert np.abs(r - 2).min() > 1e-3 and np.abs(r - 5).min() > 1e-3
    o = 0
    for S in sizes:
        rs, sg = np.sort(r[o:o + S]), np.sort(s[o:o + S])
        assert np.diff(rs).min() > 1e-3, "two rmsds of a group within 1e-3"
        assert np.diff(sg).min() > 0, "two equal scores in a group"
        o += S
