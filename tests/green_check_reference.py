"""numpy reference of the wrap-error compare (dqmc_set_green_check, include/dqmc_hip.h): the wrapped Green's function Gw against the
freshly rebuilt Gf.

  maxAbs      max |Gw - Gf| over all entries; +inf if any entry of either matrix is not finite
  argmax      row + col n of the first entry, in column-major order, that attains maxAbs (0 for an all-zero difference; the first
              non-finite entry if there is one)
  maxSiteDiag the maximum over the entries with row mod N == col mod N
  sumAbs      sum |Gw - Gf| (the mean difference is sumAbs / n^2)
  maxFresh    max |Gf|
  nonfinite   entries where either matrix is inf or NaN; they stay out of maxSiteDiag, sumAbs and maxFresh

The moduli are sqrt(re^2 + im^2) as on the device, not hypot: two roundings of the squares, one of the sum, one of the root."""
import numpy as np

U = 2.0 ** -53
# device and host differ by fused against unfused multiply-adds and one square root per modulus
TOL_MAX = 8 * U


def tol_sum(n):
    """relative tolerance of sumAbs: n^2 terms summed in a different order, each within TOL_MAX"""
    return n * n * U


def modulus(z):
    z = np.asarray(z)
    return np.sqrt(z.real * z.real + z.imag * z.imag)


def green_diff(Gw, Gf, N):
    Gw, Gf = np.asarray(Gw, dtype=np.complex128), np.asarray(Gf, dtype=np.complex128)
    n = Gf.shape[0]
    assert Gw.shape == Gf.shape == (n, n)
    bad = ~(np.isfinite(Gw.real) & np.isfinite(Gw.imag) & np.isfinite(Gf.real) & np.isfinite(Gf.imag))
    with np.errstate(invalid="ignore", over="ignore"):
        d = modulus(Gw - Gf)
        fresh = modulus(Gf)
    d_all = np.where(bad, np.inf, d)
    d_fin = np.where(bad, 0.0, d)
    row, col = np.indices((n, n))
    site = (row % N) == (col % N)
    flat = d_all.flatten(order="F")                      # column-major: index row + col n
    return dict(maxAbs=float(flat.max()), argmax=int(np.argmax(flat)), maxSiteDiag=float(np.where(site, d_fin, 0.0).max()),
                sumAbs=float(d_fin.sum()), maxFresh=float(np.where(bad, 0.0, fresh).max()), nonfinite=int(bad.sum()))


def log_spread(v):
    """log(max v / min v) of positive values"""
    v = np.asarray(v, dtype=np.float64)
    return float(np.log(v.max() / v.min()))
