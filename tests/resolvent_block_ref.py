"""Dense numpy stand-ins for the block resolvent tests: block Arnoldi with the device's deflation convention (what
nlg_basis_block_cgs2 / nlg_block_arnoldi_step hand to host._block_gmres_ls), and a complex vector / operator pair that offers
what host.resolvent_analysis touches (nek_zvector's methods, apply_linear_block)."""
import numpy as np


def block_qr_deflating(W, Q=None):
    """Columns of W orthogonalised against the orthonormal (or zero) columns of Q and among themselves, Gram-Schmidt twice.  A column
    of which less than 1e-12 of its norm is left becomes the ZERO vector with a zero row in R, as nlg_basis_block_cgs2 deflates.
    Returns (W_out, C, R) with W = Q C + W_out R, R upper triangular."""
    n, s = W.shape
    W = W.copy()
    k = 0 if Q is None else Q.shape[1]
    C = np.zeros((k, s))
    R = np.zeros((s, s))
    for v in range(s):
        full = np.linalg.norm(W[:, v])
        r = np.zeros(s)
        for _ in range(2):
            if k:
                c = Q.T @ W[:, v]
                W[:, v] -= Q @ c
                C[:, v] += c
            for u in range(v):
                c = W[:, u] @ W[:, v]
                W[:, v] -= c * W[:, u]
                r[u] += c
        nrm = np.linalg.norm(W[:, v])
        if full == 0.0 or nrm <= 1e-12 * full:
            W[:, v] = 0.0
            nrm = 0.0
        else:
            W[:, v] /= nrm
        r[v] = nrm
        R[:, v] = r
    for v in range(s):                      # a deflated column carries nothing: its row of R is zero
        if R[v, v] == 0.0:
            R[v, :] = 0.0
    return W, C, R


def block_arnoldi(A, B, nsteps):
    """nsteps block Arnoldi steps of A from the residual block B.  Returns (Q: n x (nsteps + 1) s, H: (nsteps + 1) s x nsteps s, R0)
    with B = Q[:, :s] R0 and A Q[:, :j s] = Q[:, :(j + 1) s] H[:(j + 1) s, :j s] for every j."""
    n, s = B.shape
    Q = np.zeros((n, (nsteps + 1) * s))
    H = np.zeros(((nsteps + 1) * s, nsteps * s))
    Q[:, :s], _, R0 = block_qr_deflating(B)
    for j in range(nsteps):
        k = (j + 1) * s
        W, C, R = block_qr_deflating(A @ Q[:, k - s:k], Q[:, :k])
        Q[:, k:k + s] = W
        H[:k, k - s:k] = C
        H[k:k + s, k - s:k] = R
    return Q, H, R0


class ZVec:
    """A complex vector with nek_zvector's methods (Euclidean inner product)."""

    def __init__(self, a):
        self.a = np.array(a, dtype=complex)

    def copy(self):
        return ZVec(self.a)

    def zero(self):
        self.a[:] = 0.0

    def dot(self, other):
        return complex(np.vdot(self.a, other.a))

    def norm(self):
        return float(np.linalg.norm(self.a))

    def axpby(self, alpha, vec, beta):
        self.a = complex(alpha) * vec.a + complex(beta) * self.a

    def scal(self, alpha):
        self.a = complex(alpha) * self.a

    def conj(self):
        self.a = self.a.conj()


class DenseResolvent:
    """apply_linear_block of a dense matrix M with its exact adjoint; counts the block applications."""

    def __init__(self, M):
        self.M = np.array(M, dtype=complex)
        self.napply = 0

    def apply_linear_block(self, vs, outs, adjoint=False):
        assert 1 <= len(vs) <= 4 and len(outs) == len(vs) and all(o is not v for o in outs for v in vs)
        self.napply += 1
        for v, o in zip(vs, outs):
            o.a = (self.M.conj().T if adjoint else self.M) @ v.a
