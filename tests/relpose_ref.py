"""Plain float64 numpy restatement of the relative-pose stage (test infrastructure only; does not import pnr):
five-point by SVD null space and the Stewenius action matrix, Sampson error, decomposition with the cheirality
vote of cv2.recoverPose, DLT triangulation, the pseudo-depth painting loop of include/pnr.h."""
import itertools

import numpy as np

# cubic monomials over (x, y, z, 1) = variables 0..3, degree-ordered; the last ten are the quotient basis
MONO = [(0, 0, 0), (0, 0, 1), (0, 0, 2), (0, 1, 1), (0, 1, 2), (0, 2, 2), (1, 1, 1), (1, 1, 2), (1, 2, 2), (2, 2, 2),
        (0, 0, 3), (0, 1, 3), (0, 2, 3), (1, 1, 3), (1, 2, 3), (2, 2, 3), (0, 3, 3), (1, 3, 3), (2, 3, 3), (3, 3, 3)]
W = np.array([[0., 1, 0], [-1, 0, 0], [0, 0, 1]])


def cubic(E):
    return 2 * E @ E.T @ E - np.trace(E @ E.T) * E


def five_point(x1, x2):
    """x1, x2 (5,2) with x2^T E x1 = 0 -> list of unit-norm real E"""
    Q = np.stack([np.outer(np.append(b, 1), np.append(a, 1)).ravel() for a, b in zip(x1, x2)])
    B = np.linalg.svd(Q)[2][5:].reshape(4, 3, 3)
    M = np.zeros((10, 20))
    for m, mono in enumerate(MONO):
        for p, q, r in set(itertools.permutations(mono)):   # the trilinear forms behind the two constraints
            M[:9, m] += (2 * B[p] @ B[q].T @ B[r] - np.trace(B[p] @ B[q].T) * B[r]).ravel()
            M[9, m] += np.linalg.det(np.stack([B[p][0], B[q][1], B[r][2]]))
    Bm = np.linalg.solve(M[:, :10], M[:, 10:])
    A = np.zeros((10, 10))                                   # multiplication by x on [x2 xy xz y2 yz z2 x y z 1]
    A[:6] = -Bm[:6]
    A[6, 0] = A[7, 1] = A[8, 2] = A[9, 6] = 1
    vals, vecs = np.linalg.eig(A)
    out = []
    for k in np.nonzero(np.abs(vals.imag) < 1e-9)[0]:
        v = vecs[:, k].real
        E = np.tensordot(np.append(v[6:9] / v[9], 1), B, 1)
        out.append(E / np.linalg.norm(E))
    return out


def sampson(E, x1, x2):
    h1, h2 = np.c_[x1, np.ones(len(x1))], np.c_[x2, np.ones(len(x2))]
    a, b = h1 @ E.T, h2 @ E
    return np.sum(h2 * a, 1) ** 2 / (a[:, 0] ** 2 + a[:, 1] ** 2 + b[:, 0] ** 2 + b[:, 1] ** 2)


def dlt(P1, P2, x1, x2):
    """(L,4) homogeneous points and the singular values (L,4) of each 4 x 4 system"""
    X, sv = np.zeros((len(x1), 4)), np.zeros((len(x1), 4))
    for i, (a, b) in enumerate(zip(x1, x2)):
        A = np.stack([a[0] * P1[2] - P1[0], a[1] * P1[2] - P1[1], b[0] * P2[2] - P2[0], b[1] * P2[2] - P2[1]])
        _, sv[i], vt = np.linalg.svd(A)
        X[i] = vt[3]
    return X, sv


def decompose(E, x1, x2, dist=50.0):
    """cv2.recoverPose: (R, t) of x2 ~ R x1 + t by the cheirality vote over the given matches"""
    U, _, Vt = np.linalg.svd(E)
    U, Vt = U * np.sign(np.linalg.det(U)), Vt * np.sign(np.linalg.det(Vt))
    cands = [(U @ W @ Vt, U[:, 2]), (U @ W.T @ Vt, U[:, 2]), (U @ W @ Vt, -U[:, 2]), (U @ W.T @ Vt, -U[:, 2])]
    votes = []
    for R, t in cands:
        X = dlt(np.eye(3, 4), np.c_[R, t], x1, x2)[0]
        p = X[:, :3] / X[:, 3:]
        z2 = p @ R[2] + t[2]
        votes.append(int(((p[:, 2] > 0) & (p[:, 2] < dist) & (z2 > 0) & (z2 < dist)).sum()))
    return cands[int(np.argmax(votes))]


def project(K, T, p):
    q = (K @ (T[:3, :3] @ p.T + T[:3, 3:4])).T
    return q[:, :2] / q[:, 2:], q[:, 2]


def paint(uv, depth, H, W_, patch):
    out = np.zeros((H, W_), np.float32)
    for (u, v), d in zip(uv, depth):
        if patch < v < H - patch and patch < u < W_ - patch:
            out[int(v - patch):int(v + patch), int(u - patch):int(u + patch)] = d
        elif 0 < v < H and 0 < u < W_:
            out[int(v), int(u)] = d
    return out
