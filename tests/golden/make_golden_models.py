"""Golden vectors for leg.log_likelihood_models (many models over one batch of series), recorded by running the
UNMODIFIED reference LEGFamily (cyclic_gps/models.py) in the build container:
    python tests/golden/make_golden_models.py
Writes leg_models.npz: three models (rank 3, obs_dim 2, fp64, seeds 7, 8, 9: the reference's own random initial
guesses), three series of 2, 33 and 40 rows with irregular gaps, ll[3, 3] (model, series) from one
LEGFamily.log_likelihood per pair, and for every model the gradient of ll[k, :].sum() from the reference's autograd
through its own cyclic reduction, expressed per matrix entry as make_golden_leg.record_grads does.  Arrays only.
"""
import os
import sys
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _refload  # noqa: E402

warnings.filterwarnings("ignore")

SEEDS = (7, 8, 9)
LENGTHS = (2, 33, 40)
RANK, OBS = 3, 2


def main():
    models = _refload.load_reference_models()
    g = torch.Generator().manual_seed(4242)
    ts, xs = [], []
    for n in LENGTHS:
        t0 = 20.0 * torch.rand((), dtype=torch.float64, generator=g) - 10.0          # every series on its own clock
        ts.append(t0 + torch.cumsum(torch.empty(n, dtype=torch.float64).exponential_(1.0, generator=g) + 0.01, dim=0))
        xs.append(torch.randn(n, OBS, dtype=torch.float64, generator=g).cumsum(0) * 0.1)
    out = dict(ts=torch.cat(ts).numpy(), xs=torch.cat(xs).numpy(), lengths=np.array(LENGTHS, dtype=np.int64),
               seeds=np.array(SEEDS, dtype=np.int64))
    mats = {k: [] for k in ("N", "R", "B", "Lambda", "gN", "gR", "gB", "gLambda")}
    ll = np.zeros((len(SEEDS), len(LENGTHS)))
    for k, seed in enumerate(SEEDS):
        torch.manual_seed(seed)
        m = models.LEGFamily(rank=RANK, obs_dim=OBS, train=True, data_type=torch.float64)
        m.double()
        per = [m.log_likelihood(t, x) for t, x in zip(ts, xs)]
        torch.stack(per).sum().backward()
        ll[k] = [float(v) for v in per]
        gN = torch.zeros(RANK, RANK, dtype=torch.float64)
        gN[m.N_idxs] = m.N_params.grad
        gR = torch.zeros(RANK, RANK, dtype=torch.float64)
        gR[m.R_idxs] = m.R_params.grad
        gL = torch.zeros(OBS, OBS, dtype=torch.float64)
        gL[m.Lambda_idxs] = m.Lambda_params.grad / torch.sigmoid(m.Lambda_params.detach())   # Lambda = softplus(params)
        with torch.no_grad():
            m.register_model_matrices_from_params()
        for name, val in (("N", m.N), ("R", m.R), ("B", m.B), ("Lambda", m.Lambda), ("gN", gN), ("gR", gR), ("gB", m.B.grad),
                          ("gLambda", gL)):
            mats[name].append(val.detach().numpy().copy())
    out.update({name: np.stack(v) for name, v in mats.items()})
    out["ll"] = ll
    np.savez_compressed(os.path.join(HERE, "leg_models.npz"), **out)
    print("wrote leg_models.npz", ll)


if __name__ == "__main__":
    main()
