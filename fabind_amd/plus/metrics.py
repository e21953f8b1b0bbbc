"""FABind+ confidence metrics and top-N selection without per-pair host synchronisation.

`ConfidenceEvaluator` accumulates what the reference's confidence loops accumulate (FABind_plus/fabind/utils/training_confidence.py
:215-326 -- validation; :41-149 is the same bookkeeping around the training step) and returns the dictionary of :313-326.  The
reference appends one python float per PAIR of copies (`ranking_accuracy_list`, a `.item()`-style read per pair) and reads three
losses back per batch; here the ranking kernel (csrc/ranking.hip) returns the four counts of a group, the partial sums stay on the
device, and `compute()` reads everything back in one transfer.

`select_by_confidence` / `sampling_metrics` are the top-N evaluation of test_sampling_fabind.py:159-191 (FABind+'s sampling table)
on [S, B] tensors instead of S text files; they run once per evaluation and are plain torch.

`select_distinct_by_confidence` / `distinct_sampling_metrics` are the same evaluation over DISTINCT poses: the leaders of the first
`top_n` clusters of `fabind_amd.poses.cluster_poses` instead of the `top_n` most confident samples, which are usually one binding mode
several times.

`select_valid_by_confidence` / `valid_sampling_metrics` are the same evaluation with the physical validity of every pose
(`fabind_amd.validity.check_poses`) taken into account: valid poses are chosen first, and the table gains the "RMSD < 2 A and valid"
column docking benchmarks report."""
import torch

from .models.model import confidence_terms


def _summary(x, prefix):
    q = [torch.quantile(x, p) for p in (0.25, 0.50, 0.75)]
    return [prefix, prefix + " < 2A", prefix + " < 5A", prefix + " 25%", prefix + " 50%", prefix + " 75%"], \
        [x.mean(), (x < 2).float().mean(), (x < 5).float().mean()] + q


class ConfidenceEvaluator:
    """`update` once per batch with the model's 7-tuple, `compute` once at the end.  `update` issues no host synchronisation,
    `compute` exactly one.  args: `ranking_loss` (logsigmoid / dynamic_hinge) and `keep_cls_2A`, as compute_confidence_loss reads them.

    The reference's conventions are kept as they are: the three losses are averaged with weight len(scores) per batch;
    `confidence_accuracy` compares the FIRST score of a group with every copy's [rmsd < 2 A] (training_confidence.py:252);
    `hit_rate` and `confidence_accuracy` divide by the number of samples, `ranking_accuracy` by the number of pairs."""

    def __init__(self, args=None):
        self.mode = getattr(args, "ranking_loss", "logsigmoid") if args is not None else "logsigmoid"
        self.with_ce = bool(getattr(args, "keep_cls_2A", False)) if args is not None else False
        self.reset()

    def reset(self):
        self._rmsd, self._cdis = [], []
        self._loss = None            # float64 [3]: sum of len(scores) * (loss, ranking, ce)
        self._count = None           # int64 [5]: ranked_right, pairs, hit, confidence_correct, skipped samples
        self.samples = self.less5 = 0

    @torch.no_grad()
    def update(self, out, coords_true, group_size=None, rmsd=None):
        loss, info = confidence_terms(out, coords_true, self.mode, self.with_ce, group_size, rmsd)
        logits, mask = out[2], out[3]
        B = info["rmsd"].shape[0]
        # training_confidence.py:272-279: a sample whose pocket head predicts no residue at all
        skipped = (((logits.sigmoid().round() == 1) & mask.bool()).sum(1) == 0).sum()
        part = torch.stack([loss, info["ranking"], info["ce"]]).double() * B
        cnt = torch.cat([info["counts"].sum(0, dtype=torch.int64), skipped.reshape(1)])
        self._loss = part if self._loss is None else self._loss + part
        self._count = cnt if self._count is None else self._count + cnt
        self._rmsd.append(info["rmsd"])
        self._cdis.append(info["centroid_dis"])
        self.samples += int(mask.shape[0])
        self.less5 += int(out[4])
        return loss

    def compute(self):
        if not self._rmsd:
            raise RuntimeError("ConfidenceEvaluator.compute: no batch has been added")
        rmsd, cdis = torch.cat(self._rmsd), torch.cat(self._cdis)
        names_r, vals_r = _summary(rmsd, "rmsd")
        names_c, vals_c = _summary(cdis, "centroid_dis")
        flat = torch.cat([torch.stack(vals_r + vals_c).double(), self._loss, self._count.double()]).tolist()   # the one read-back
        n = rmsd.shape[0]
        metrics = {"samples": self.samples, "skip_samples": int(flat[-1]), "keepNode < 5": self.less5}
        metrics.update(zip(names_r + names_c, flat[:12]))
        tot, ranking, ce = flat[12:15]
        right, pairs, hit, conf = flat[15:19]
        metrics.update({"confidence_loss": tot / n, "ranking_loss": ranking / n, "confidence_ce_loss": ce / n,
                        "confidence_accuracy": conf / n, "ranking_accuracy": right / pairs if pairs > 0 else 0.,
                        "hit_rate": hit / n})
        return metrics


def select_by_confidence(rmsd, cdis, conf, top_n=1):
    """test_sampling_fabind.py:163-175: per complex, among its `top_n` most confident samples, the minimum RMSD and the minimum
    centroid distance (each minimum on its own, as the reference takes them).  rmsd, cdis, conf: [S, B] (S samples of B complexes).
    -> (rmsd [B], centroid distance [B]).  Equal confidences keep their sample order."""
    if rmsd.dim() != 2 or tuple(cdis.shape) != tuple(rmsd.shape) or tuple(conf.shape) != tuple(rmsd.shape):
        raise ValueError("select_by_confidence: rmsd, cdis and conf must share one [S, B] shape; got %s, %s, %s"
                         % (tuple(rmsd.shape), tuple(cdis.shape), tuple(conf.shape)))
    if not 1 <= int(top_n) <= rmsd.shape[0]:
        raise ValueError("select_by_confidence: top_n must be in [1, S = %d]; got %r" % (rmsd.shape[0], top_n))
    pick = torch.argsort(conf, dim=0, descending=True, stable=True)[:int(top_n)]
    return rmsd.gather(0, pick).min(0).values, cdis.gather(0, pick).min(0).values


def sampling_metrics(rmsd, cdis, conf, top_n=1):
    """test_sampling_fabind.py:177-191 on the selection above: mean, the < 2 A and < 5 A rates and the quartiles of the selected
    RMSD and centroid distance.  The rates divide by B (the reference hard-codes its test set's 363).  -> dict of python floats."""
    r, c = select_by_confidence(rmsd, cdis, conf, top_n)
    vals, names = [], []
    for x, p in ((r.double(), "rmsd"), (c.double(), "centroid_dis")):
        names += [p + s for s in ("_mean", "_2A", "_5A", "_25", "_50", "_75")]
        vals += [x.mean(), (x < 2).double().mean(), (x < 5).double().mean()] + [torch.quantile(x, q) for q in (0.25, 0.50, 0.75)]
    return dict(zip(names, torch.stack(vals).tolist()))


def select_distinct_by_confidence(rmsd, cdis, conf, clusters, top_n=1):
    """`select_by_confidence` over distinct poses: per complex the minimum RMSD and the minimum centroid distance among the leaders of
    its first `top_n` clusters (`clusters`: the `poses.PoseClusters` of the same [S, B] samples, clusters in the confidence order of
    their leaders).  A complex with fewer than `top_n` clusters uses the clusters it has.
    -> (rmsd [B], centroid distance [B], the chosen pose indices int64 [top_n, B], -1 where a complex has no such cluster)."""
    if rmsd.dim() != 2 or tuple(cdis.shape) != tuple(rmsd.shape) or tuple(conf.shape) != tuple(rmsd.shape) or \
            tuple(clusters.leader.shape) != tuple(rmsd.shape):
        raise ValueError("select_distinct_by_confidence: rmsd, cdis, conf and clusters.leader must share one [S, B] shape; got %s, %s, %s, %s"
                         % (tuple(rmsd.shape), tuple(cdis.shape), tuple(conf.shape), tuple(clusters.leader.shape)))
    if not 1 <= int(top_n) <= rmsd.shape[0]:
        raise ValueError("select_distinct_by_confidence: top_n must be in [1, S = %d]; got %r" % (rmsd.shape[0], top_n))
    pick = clusters.leader[:int(top_n)].long()
    have, at = pick >= 0, pick.clamp(min=0)
    inf = torch.full_like(rmsd[:1], float("inf"))
    return (torch.where(have, rmsd.gather(0, at), inf).min(0).values, torch.where(have, cdis.gather(0, at), inf).min(0).values, pick)


def distinct_sampling_metrics(rmsd, cdis, conf, clusters, top_n=1):
    """The dictionary of `sampling_metrics` on `select_distinct_by_confidence`, plus `n_clusters_mean` (clusters per complex) and
    `top_cluster_share` (the mean over complexes of the population of cluster 0 over S: how much of the sampling agrees with the most
    confident pose).  -> dict of python floats, one read-back."""
    r, c, _ = select_distinct_by_confidence(rmsd, cdis, conf, clusters, top_n)
    vals, names = [], []
    for x, p in ((r.double(), "rmsd"), (c.double(), "centroid_dis")):
        names += [p + s for s in ("_mean", "_2A", "_5A", "_25", "_50", "_75")]
        vals += [x.mean(), (x < 2).double().mean(), (x < 5).double().mean()] + [torch.quantile(x, q) for q in (0.25, 0.50, 0.75)]
    names += ["n_clusters_mean", "top_cluster_share"]
    vals += [clusters.n_clusters.double().mean(), clusters.size[0].double().mean() / rmsd.shape[0]]
    return dict(zip(names, torch.stack(vals).tolist()))


def _valid_picks(rmsd, cdis, conf, valid, top_n, who):
    if rmsd.dim() != 2 or any(tuple(t.shape) != tuple(rmsd.shape) for t in (cdis, conf, valid)):
        raise ValueError("%s: rmsd, cdis, conf and valid must share one [S, B] shape; got %s, %s, %s, %s"
                         % (who, tuple(rmsd.shape), tuple(cdis.shape), tuple(conf.shape), tuple(valid.shape)))
    if not 1 <= int(top_n) <= rmsd.shape[0]:
        raise ValueError("%s: top_n must be in [1, S = %d]; got %r" % (who, rmsd.shape[0], top_n))
    order = torch.argsort(conf, dim=0, descending=True, stable=True)
    invalid = (~valid.bool().gather(0, order)).to(torch.int8)
    return order.gather(0, torch.argsort(invalid, dim=0, stable=True))[:int(top_n)]


def select_valid_by_confidence(rmsd, cdis, conf, valid, top_n=1):
    """`select_by_confidence` among the VALID poses of each complex: per complex the minimum RMSD and the minimum centroid distance among
    its `top_n` most confident valid samples; a complex with fewer than `top_n` valid samples is filled with its most confident invalid
    ones.  rmsd, cdis, conf, valid: [S, B] (`validity.check_poses(...).valid.t()`); equal confidences keep their sample order.
    -> (rmsd [B], centroid distance [B])."""
    pick = _valid_picks(rmsd, cdis, conf, valid, top_n, "select_valid_by_confidence")
    return rmsd.gather(0, pick).min(0).values, cdis.gather(0, pick).min(0).values


def valid_sampling_metrics(rmsd, cdis, conf, valid, top_n=1):
    """The dictionary of `sampling_metrics` on `select_valid_by_confidence`, plus `valid_share` (valid poses over all S * B poses),
    `top1_valid_share` (complexes whose most confident pose is valid) and `rmsd_lt2_and_valid` (complexes with a chosen pose that is
    valid and below 2 A: the "RMSD < 2 A and physically valid" column).  -> dict of python floats, one read-back."""
    pick = _valid_picks(rmsd, cdis, conf, valid, top_n, "valid_sampling_metrics")
    v = valid.bool()
    r, c = rmsd.gather(0, pick).min(0).values, cdis.gather(0, pick).min(0).values
    vals, names = [], []
    for x, p in ((r.double(), "rmsd"), (c.double(), "centroid_dis")):
        names += [p + s for s in ("_mean", "_2A", "_5A", "_25", "_50", "_75")]
        vals += [x.mean(), (x < 2).double().mean(), (x < 5).double().mean()] + [torch.quantile(x, q) for q in (0.25, 0.50, 0.75)]
    top1 = torch.argsort(conf, dim=0, descending=True, stable=True)[:1]
    names += ["valid_share", "top1_valid_share", "rmsd_lt2_and_valid"]
    vals += [v.double().mean(), v.gather(0, top1).double().mean(), (v.gather(0, pick) & (rmsd.gather(0, pick) < 2)).any(0).double().mean()]
    return dict(zip(names, torch.stack(vals).tolist()))


def energy_sampling_metrics(rmsd, cdis, energy, valid=None, top_n=1):
    """The sampling table with a physics-based energy as the ranking signal (`fabind_amd.scoring.score_poses(...).total.t()`; lower is
    better) where no confidence model exists: `sampling_metrics` (valid=None) or `valid_sampling_metrics` called with conf = -energy.
    A pose without an energy (NaN: NONFINITE or UNCHECKED) ranks last.  rmsd, cdis, energy (and valid): [S, B].
    -> dict of python floats."""
    conf = torch.where(torch.isnan(energy), torch.full_like(energy, float("-inf")), -energy)
    if valid is None:
        return sampling_metrics(rmsd, cdis, conf, top_n)
    return valid_sampling_metrics(rmsd, cdis, conf, valid, top_n)
