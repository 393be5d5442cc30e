"""Dense numpy statement of the reference's three unsymmetric Newton matrices, written from the
formulas (not from the product code); the yardstick for sizes the recorded fixtures do not reach.

With ``A`` = active set, ``I`` = inactive set (ascending), ``lamb = 1 / dt``,
``Hl = H + lamb I_n``, ``delta = lamb / (1 + lamb rho)``:

* Standard   (standard_step_solver.py:40-92, ImplicitFunc.deriv), natural order; ``H`` carries the
  ``rho J'J`` term: row ``i in I``: ``[e_i + dt H[i,:], dt J[:,i]']``; row ``i in A``: ``e_i``;
  constraint rows ``[-dt J, I_m]``.
* Extended   (extended_step_solver.py:39-112): ``|A|`` unit rows ``e_a``, then
  ``[Hl[I,:], J[:,I]']``, then ``[J, -delta I_m]``.
* Asymmetric (asymmetric_step_solver.py:38-173): ``[[Hl, J'], [J, -delta I_m]]`` with every
  active row overwritten by ``e_a``.
"""

import numpy as np


def newton_matrix(form, H, J, mask, dt, rho):
    H = np.asarray(H, dtype=np.float64)
    mask = np.asarray(mask, dtype=bool)
    n = mask.size
    J = np.asarray(J, dtype=np.float64).reshape(-1, n)
    m = J.shape[0]
    lamb = 1.0 / dt
    delta = lamb / (1.0 + lamb * rho)
    act, ina = np.where(mask)[0], np.where(~mask)[0]
    M = np.zeros((n + m, n + m))
    if form == "Standard":
        M[:n, :n] = dt * H
        M[:n, n:] = dt * J.T
        M[act, :] = 0.0
        M[np.arange(n), np.arange(n)] += 1.0
        M[n:, :n] = -dt * J
        M[n:, n:] = np.eye(m)
    elif form == "Extended":
        Hl = H + lamb * np.eye(n)
        M[np.arange(act.size), act] = 1.0
        M[act.size:n, :n] = Hl[ina, :]
        M[act.size:n, n:] = J[:, ina].T
        M[n:, :n] = J
        M[n:, n:] = -delta * np.eye(m)
    elif form == "Asymmetric":
        M[:n, :n] = H + lamb * np.eye(n)
        M[:n, n:] = J.T
        M[n:, :n] = J
        M[n:, n:] = -delta * np.eye(m)
        M[act, :] = 0.0
        M[act, act] = 1.0
    else:
        raise ValueError(form)
    return M
