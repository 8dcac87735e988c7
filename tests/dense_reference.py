"""An independent statement of the decode's HMM in float64: the dense K x K transition matrix built from (D, B, U,
rowRatios, columnRatios) (Transition.java:152-209) and a textbook forward-backward, in array and
sequence mode.  Used by tests/test_oracle_dense.py and tests/test_oracle_dense_edges.py."""
import numpy as np


def dense_T(m, row):
    K = m.K
    D, B, U, RR, cR = (x.astype(np.float64) for x in (m.D[row], m.B[row], m.U[row], m.RR[row], m.col_ratios))
    T = np.zeros((K, K))
    for i in range(K):
        T[i, i] = D[i]
        T[i, :i] = B[:i]
    for i in range(K - 2, -1, -1):
        # T[i, j] = T[i, j - 1] * cR[j - 1] for j > i + 1: a running product, left to right (np.cumprod)
        T[i, i + 1:] = np.cumprod(np.concatenate([[U[i]], cR[i + 1:K - 1]]))
    # the row-ratio form must describe the same matrix
    upper = np.triu(np.ones((K - 2, K), bool), 2)
    np.testing.assert_allclose(T[:K - 2][upper], (RR[:K - 2, None] * T[1:K - 1])[upper], rtol=2e-5, atol=1e-30)
    return T


def emission(m, pos, x, a):
    z, t = (0.0 if x else 1.0), (1.0 if a else 0.0)
    return m.e1[pos].astype(np.float64) + m.e0m1[pos].astype(np.float64) * z + m.e2m0[pos].astype(np.float64) * t


def dense_posterior(m, xbits, abits, frm, to):
    K = m.K
    n = to - frm
    al = np.zeros((n, K))
    be = np.zeros((n, K))
    a = m.pi.astype(np.float64) * emission(m, frm, xbits[0], abits[0])
    al[0] = a / a.sum()
    Ts = {}
    for p in range(frm + 1, to):
        T = Ts.setdefault(int(m.step_row[p]), dense_T(m, int(m.step_row[p])))
        a = emission(m, p, xbits[p - frm], abits[p - frm]) * (al[p - frm - 1] @ T)
        al[p - frm] = a / a.sum()
    be[n - 1] = 1.0 / K
    for p in range(to - 2, frm - 1, -1):
        T = Ts[int(m.step_row[p + 1])]
        b = T @ (emission(m, p + 1, xbits[p + 1 - frm], abits[p + 1 - frm]) * be[p + 1 - frm])
        be[p - frm] = b / b.sum()
    post = al * be
    return post / post.sum(axis=1, keepdims=True)


def dense_posterior_sequence(m, xbits, abits, frm, to):
    """Sequence mode as the reference's buffers end up (HMM.cpp:760-770, 915-925 and hmm_oracle.h): the stored
    alpha of site p < to-1 is the un-scaled vector after the homozygous half-step towards p+1, the stored beta of
    site p > from the one after the half-step towards p-1."""
    K = m.K
    n = to - frm
    Ts = {}

    def T(row):
        return Ts.setdefault(int(row), dense_T(m, int(row)))

    hom = m.hom.astype(np.float64)
    al = np.zeros((n, K))
    be = np.zeros((n, K))
    a = m.pi.astype(np.float64) * emission(m, frm, xbits[0], abits[0])
    a /= a.sum()
    for p in range(frm + 1, to):
        half = hom[p] * (a @ T(m.gap_row_f[p]))
        al[p - 1 - frm] = half
        a = emission(m, p, xbits[p - frm], abits[p - frm]) * (half @ T(m.site_row_f[p]))
        a /= a.sum()
    al[n - 1] = a
    b = np.full(K, 1.0 / K)
    for p in range(to - 2, frm - 1, -1):
        q = p + 1
        half = T(m.gap_row_b[q]) @ (hom[q] * b)
        be[q - frm] = half
        b = T(m.site_row_b[q]) @ (emission(m, q, xbits[q - frm], abits[q - frm]) * half)
        b /= b.sum()
    be[0] = b
    post = al * be
    return post / post.sum(axis=1, keepdims=True)
