"""Float64 restatement of the distance-map pose generation (csrc/distgen.hip), written from its formulas with torch autograd and
torch.optim.Adam; the reference every distgen test compares against.  Also the synthetic cases the tests share.

  dis = min(|p_i - x_k|, 10), r = dis - y[i, k]
  interaction   = sum |r| (mode 0) | sum r^2 (mode 1) | sum (|r| + 1e-5)^0.5 (mode 2)
  configuration = sum_{mask} | |x_k - x_j| - D_kj | + 2 sum_{k,j} relu(1.22 - |x_k - x_j|)      (mask given)
                = sum_{k,j}  | |x_k - x_j| - D_kj |                                              (mask None)
  loss_t = interaction (t < config_start) else interaction + config_rate (t - config_start) configuration"""
import numpy as np
import torch

F64 = torch.float64


def _cdist(a, b):
    return torch.cdist(a, b, compute_mode="donot_use_mm_for_euclid_dist")


def interaction_term(x, y, pocket, mode):
    r = (_cdist(pocket, x).clamp(max=10) - y).abs()
    return r.sum() if mode == 0 else (r ** 2).sum() if mode == 1 else ((r + 1e-5) ** 0.5).sum()


def configuration_term(x, D, mask):
    own = _cdist(x, x)
    dev = (own - D).abs()
    if mask is None:
        return dev.sum()
    return dev[mask].sum() + 2 * (1.22 - own).relu().sum()


def configuration_from_lists(x, ptr, idx, dist, excluded_volume):
    """The same term from the kernel's constraint lists: every entry (owner k, other j, D) weighs 1/2."""
    owner = torch.repeat_interleave(torch.arange(x.shape[0]), (ptr[1:] - ptr[:-1]).long())
    d = (x[owner] - x[idx.long()]).norm(dim=-1)
    out = 0.5 * (d - dist).abs().sum()
    if excluded_volume:
        out = out + 2 * (1.22 - _cdist(x, x)).relu().sum()
    return out


def restate(x0, y, pocket, D, mask, epochs, mode=0, config_start=500, config_rate=5e-3, truth=None, lr=0.1):
    """-> dict(x [n, 3], loss / inter / config / rmsd [epochs]) in float64.  loss / inter / config are evaluated before the
    epoch's step, rmsd (to `truth`) after it."""
    t64 = lambda a: None if a is None else torch.as_tensor(a).to(F64)
    y, pocket, D, truth = t64(y), t64(pocket), t64(D), t64(truth)
    mask = None if mask is None else torch.as_tensor(mask).bool()
    x = t64(x0).clone().requires_grad_(True)
    opt = torch.optim.Adam([x], lr=lr)
    out = dict(loss=[], inter=[], config=[], rmsd=[])
    for t in range(epochs):
        opt.zero_grad()
        inter, config = interaction_term(x, y, pocket, mode), configuration_term(x, D, mask)
        loss = inter if t < config_start else inter + config_rate * (t - config_start) * config
        loss.backward()
        opt.step()
        out["loss"].append(loss.item()); out["inter"].append(inter.item()); out["config"].append(config.item())
        out["rmsd"].append(float("nan") if truth is None else ((truth - x.detach()) ** 2).sum(-1).mean().sqrt().item())
    res = {k: np.asarray(v) for k, v in out.items()}
    res["x"] = x.detach().numpy().copy()
    return res


# ---- the synthetic cases: random-walk chains with 1.5 A steps, pocket points ~ N(0, 8 A), LAS mask |i - j| <= 2 ----
def chain(n, gen):
    step = torch.randn(n, 3, generator=gen, dtype=F64)
    step = 1.5 * step / step.norm(dim=-1, keepdim=True)
    x = torch.cumsum(step, 0)
    return x - x.mean(0)


def synthetic(P, n, seed, noise=0.0):
    """-> dict of float32 numpy arrays: pocket [P, 3], coords [n, 3] (true pose), y [P, n], D [n, n], mask [n, n] bool."""
    gen = torch.Generator().manual_seed(seed)
    pocket = 8.0 * torch.randn(P, 3, generator=gen, dtype=F64)
    coords = chain(n, gen)
    y = _cdist(pocket, coords).clamp(max=10)
    if noise:
        y = (y + noise * torch.randn(P, n, generator=gen, dtype=F64)).clamp(min=0)
    i = torch.arange(n)
    mask = (i[:, None] - i[None, :]).abs() <= 2
    f = lambda a: a.to(torch.float32).numpy()
    return dict(pocket=f(pocket), coords=f(coords), y=f(y), D=f(_cdist(coords, coords)), mask=mask.numpy())


def start(pocket, n, seed):
    """The reference's start for torch.manual_seed(seed): 5 (2 u - 1) + the pocket's mean, u = torch.rand([n, 3]) in float32."""
    pocket = torch.as_tensor(pocket)
    torch.manual_seed(seed)
    return (5 * (2 * torch.rand(n, 3) - 1) + pocket.mean(axis=0).reshape(1, 3)).numpy()
