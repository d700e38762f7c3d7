"""Golden vectors for predict.make_predictions_models / predictive_posterior_models (many models over one batch of
series), recorded by running the UNMODIFIED reference LEGFamily (cyclic_gps/models.py) in the build container:
    python tests/golden/make_golden_models_predictions.py
Reads leg_models.npz (make_golden_models.py: three models of rank 3 and obs_dim 2, seeds 7, 8, 9; three series of 2, 33
and 40 rows) and rebuilds the same three reference models from their seeds (their matrices are checked against the
file).  Writes leg_models_predictions.npz: the models' matrices, the series, a few dozen targets per series (before the
first row, at it, between rows, on rows, at the last row and after it) and, per (model, series), the reference's
predictive_posterior (pp_mean, pp_cov) and make_predictions (pred_mean, pred_cov), one call each, concatenated over the
series in the order of target_ts: arrays [3, P, ...].  Arrays only.
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

RANK, OBS = 3, 2


def targets(ts):
    n = ts.shape[0]
    mid = 0.5 * (ts[:-1] + ts[1:])
    parts = [ts[:1] - 2.0, ts[:1], mid[:24], ts[n // 2:n // 2 + 2], ts[-1:], ts[-1:] + 0.75, ts[-1:] + 6.0]
    return torch.unique(torch.cat(parts))


def main():
    models = _refload.load_reference_models()
    src = np.load(os.path.join(HERE, "leg_models.npz"))
    lengths = [int(n) for n in src["lengths"]]
    ts_all, xs_all = torch.from_numpy(src["ts"]), torch.from_numpy(src["xs"])
    ts, xs, s = [], [], 0
    for n in lengths:
        ts.append(ts_all[s:s + n])
        xs.append(xs_all[s:s + n])
        s += n
    tts = [targets(t) for t in ts]
    keys = ("pp_mean", "pp_cov", "pred_mean", "pred_cov")
    rec = {k: [] for k in keys}
    for k, seed in enumerate(int(v) for v in src["seeds"]):
        torch.manual_seed(seed)
        m = models.LEGFamily(rank=RANK, obs_dim=OBS, train=True, data_type=torch.float64)
        m.double()
        with torch.no_grad():
            m.register_model_matrices_from_params()
            for name, val in (("N", m.N), ("R", m.R), ("B", m.B), ("Lambda", m.Lambda)):
                assert np.array_equal(val.detach().numpy(), src[name][k]), (seed, name)
            per = {key: [] for key in keys}
            for t, x, tt in zip(ts, xs, tts):
                pp_mean, pp_cov = m.predictive_posterior(t, x, tt)
                p_mean, p_cov = m.make_predictions(t, x, tt)
                for key, val in zip(keys, (pp_mean, pp_cov, p_mean, p_cov)):
                    per[key].append(val.detach().numpy())
        for key in keys:
            rec[key].append(np.concatenate(per[key]))
    out = {key: np.stack(v) for key, v in rec.items()}
    out.update({name: src[name] for name in ("N", "R", "B", "Lambda", "ts", "xs", "lengths", "seeds")})
    out["target_ts"] = torch.cat(tts).numpy()
    out["target_lengths"] = np.array([int(t.shape[0]) for t in tts], dtype=np.int64)
    np.savez_compressed(os.path.join(HERE, "leg_models_predictions.npz"), **out)
    print("wrote leg_models_predictions.npz", out["target_lengths"], {k: out[k].shape for k in keys})


if __name__ == "__main__":
    main()
