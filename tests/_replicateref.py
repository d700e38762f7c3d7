"""float64 restatement of the replicated observations of one LEG series under one model, written from
the definition:

    x[r, c, s] = sum_j B[c, j] z[r, j, s] + sum_c' T_r[c, c'] eps''_r[c', s],   T_r T_r^T = LLT + diag(s_r),  T_r lower,

s_r[c] the row's noise variance where the entry is observed and 0 elsewhere (whatever the array holds there).  The mask
only selects variances: every row and channel gets a value.  eps''_r[c'] is element (id 2^40 + r obs + c', column s) of
the generator (tests/_rngref.py) under stream word `stream + 2`; the latent noise of a draw of the same series uses
`stream`, its observation noise `stream + 1` (tests/_perturbref.py), and model k of a `*_models` call has
stream = stream0 + 4 k by default.  Everything dense, per series, numpy float64."""
import numpy as np

import _perturbref as pr
import _rngref

model = pr.model                                  # (G, B, LLT) from the four model matrices
WORDS_PER_MODEL = 4


def draw_words(stream):
    """The three stream words of one model's draw: latent noise, observation noise of the perturbation, replicate."""
    return [int(stream), int(stream) + 1, int(stream) + 2]


def default_model_streams(M, stream=0):
    return [int(stream) + WORDS_PER_MODEL * k for k in range(M)]


def row_variances(n, obs, observed=None, s=None):
    """s_r [n, obs]: the variances where observed, 0 elsewhere."""
    observed = np.ones((n, obs), dtype=bool) if observed is None else np.asarray(observed, dtype=bool).reshape(n, -1)
    observed = np.broadcast_to(observed, (n, obs))
    s = np.zeros((n, obs)) if s is None else np.broadcast_to(np.asarray(s, dtype=np.float64).reshape(n, -1), (n, obs))
    return np.where(observed, s, 0.0)


def replicate_from_noise(Bm, LLT, z, eps2, observed=None, s=None):
    """x [n, obs, S] from z [n, d, S] and eps'' [n, obs, S]."""
    n, obs = z.shape[0], Bm.shape[0]
    sv = row_variances(n, obs, observed, s)
    x = np.empty((n, obs, z.shape[2]))
    for r in range(n):
        x[r] = Bm @ z[r] + np.linalg.cholesky(LLT + np.diag(sv[r])) @ eps2[r]
    return x


def noise(n, obs, sid, S, seed, stream=0, dtype=np.float64):
    return _rngref.standard_normal(n * obs, S, seed, stream + 2, dtype, row0=int(sid) << 40).reshape(n, obs, S)


def replicates(Bm, LLT, z, sid, seed, stream=0, observed=None, s=None, dtype=np.float64):
    """x [n, obs, S] of one series with id `sid` given its paths z [n, d, S]; `dtype` names the generator (fp64 or fp32
    uniforms), the arithmetic is float64 either way."""
    z = np.asarray(z, dtype=np.float64)
    return replicate_from_noise(Bm, LLT, z, noise(z.shape[0], Bm.shape[0], sid, z.shape[2], seed, stream, dtype), observed, s)
