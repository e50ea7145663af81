"""numpy fp64 restatement of mvg_structural_triangulate (csrc/structural.hip, contract in include/mvg_decoder.h), operation for
operation: every product is rounded on its own, every sum is an explicit accumulation in ascending index order from +0.0, the
factorisations use the header's elimination order.  Vectorised over the persons only (the leading axis); a term that the kernel
does not form (below a triangle's start) enters here as +0.0, which changes no bit of a chain that starts at +0.0 or subtracts.

    solve(ud, conf, Pm, parent, bone_len, method, n_steps)          the persons of one list
    dense(ud, conf, Pm, parent, bone_len, valid, ...)               the kernel's dense addressing, (B, NQ) persons
    by_rows(ud, conf, Pm, parent, bone_len, rows, count, ...)       the kernel's rows addressing, (B, R) persons
"""
import numpy as np

LS, ST = 0, 1
METHODS = {"LS": LS, "ST": ST}


def ancestors(parent):
    """anc[i] = set of the bones (named by their end joint k >= 1) on the path root -> i"""
    J = len(parent)
    assert parent[0] == -1
    anc = []
    for i in range(J):
        s, j = set(), i
        for _ in range(J):
            if j == 0:
                break
            s.add(j)
            j = int(parent[j])
        assert j == 0, "parent is not a tree rooted at joint 0"
        anc.append(s)
    return anc


def chol(A):
    """lower Cholesky factor, column by column; A (N, n, n), the lower triangle is read -> (L, ok (N) bool)"""
    N, n, _ = A.shape
    L = np.zeros_like(A)
    ok = np.ones(N, bool)
    for j in range(n):
        s = A[:, j:, j].copy()
        for k in range(j):
            s = s - L[:, j:, k] * L[:, j, k, None]
        piv = s[:, 0]
        ok &= piv > 0
        d = np.sqrt(piv)
        L[:, j, j] = d
        L[:, j + 1:, j] = s[:, 1:] / d[:, None]
    return L, ok


def inv_from_chol(L):
    """Y = L^-1 by forward substitution (a column of the identity at a time), then Y^T Y"""
    N, n, _ = L.shape
    Y = np.zeros_like(L)
    eye = np.eye(n)
    for i in range(n):
        s = np.broadcast_to(eye[i], (N, n)).copy()
        for k in range(i):
            s = s - L[:, i, k, None] * Y[:, k, :]
        Y[:, i, :] = s / L[:, i, i, None]
    Y = Y * np.tri(n)[None]                       # column c starts at row c: what lies above is not formed
    Y = Y + 0.0                                   # -0.0 (0 * negative) -> +0.0
    Inv = np.zeros_like(L)
    for k in range(n):
        Inv = Inv + Y[:, k, :, None] * Y[:, k, None, :]
    return Inv


def _mirror(M):
    lo = np.tril(M)
    return lo + np.swapaxes(np.tril(M, -1), 1, 2)


def _matvec(M, x):
    acc = np.zeros(M.shape[:2])
    for c in range(M.shape[2]):
        acc = acc + M[:, :, c] * x[:, c, None]
    return acc


def solve(ud, conf, Pm, parent, bone_len, method="ST", n_steps=1, full=False):
    """ud (N, V, J, 2), conf (N, V, J) or None, Pm (N, V, 3, 4), bone_len (N, J-1) (ignored for LS), all fp32 values
    -> X (N, J, 3) fp32, status (N) int32 in {0, 1, 2}; full: also X before its one rounding to fp32 (fp64)"""
    method = METHODS.get(method, method)
    ud = np.asarray(ud, np.float32).astype(np.float64)
    Pm = np.asarray(Pm, np.float32).astype(np.float64)
    N, V, J, _ = ud.shape
    K, n = J - 1, 3 * (J - 1)
    anc = ancestors(parent)
    if conf is None:
        cf = np.full((N, V, J), 1.0 / float(V))
    else:
        cf = np.asarray(conf, np.float32).astype(np.float64)
    with np.errstate(all="ignore"):
        # 1. per joint: D (sym 3 x 3), m
        D = np.zeros((N, J, 3, 3))
        m = np.zeros((N, J, 3))
        for v in range(V):
            u, w = ud[:, v, :, 0], ud[:, v, :, 1]                                     # (N, J)
            r0, r1, r2 = (Pm[:, v, None, i, :3] for i in range(3))                    # (N, 1, 3)
            t0, t1, t2 = (Pm[:, v, None, i, 3] for i in range(3))                     # (N, 1)
            g0 = r0 - u[..., None] * r2
            g1 = r1 - w[..., None] * r2
            h0 = t0 - u * t2
            h1 = t1 - w * t2
            c2 = 2.0 * cf[:, v, :]
            D = D + c2[..., None, None] * (g0[..., :, None] * g0[..., None, :] + g1[..., :, None] * g1[..., None, :])
            m = m - c2[..., None] * (g0 * h0[..., None] + g1 * h1[..., None])
        # 2. tree sums
        T = np.zeros((N, 3, 3))
        mu = np.zeros((N, 3))
        for i in range(J):
            T = T + D[:, i]
            mu = mu + m[:, i]
        C = np.zeros((N, K, 3, 3))
        cm = np.zeros((N, K, 3))
        for k in range(1, J):
            for i in range(J):
                if k in anc[i]:
                    C[:, k - 1] = C[:, k - 1] + D[:, i]
                    cm[:, k - 1] = cm[:, k - 1] + m[:, i]
        LT, okT = chol(T)
        Tinv = inv_from_chol(LT)
        W = np.zeros((N, K, 3, 3))
        for k in range(K):
            for c in range(3):
                W[:, k] = W[:, k] + Tinv[:, :, c, None] * C[:, k, c, None, :]
        tm = _matvec(Tinv, mu)
        A = np.zeros((N, n, n))
        beta = np.zeros((N, n))
        for k in range(1, J):
            beta[:, 3 * (k - 1):3 * k] = cm[:, k - 1] - _matvec(C[:, k - 1], tm)
            for l in range(1, J):
                acc = np.zeros((N, 3, 3))
                for c in range(3):
                    acc = acc + C[:, k - 1, :, c, None] * W[:, l - 1, c, None, :]
                if k in anc[l]:
                    base = C[:, l - 1]
                elif l in anc[k]:
                    base = C[:, k - 1]
                else:
                    base = np.zeros((N, 3, 3))
                A[:, 3 * (k - 1):3 * k, 3 * (l - 1):3 * l] = base - acc
        # 3. Inv = A^-1, b = Inv beta
        LA, okA = chol(A)
        Inv = inv_from_chol(LA)
        b = _matvec(Inv, beta)
        status = np.where(okT & okA, 0, 1).astype(np.int32)
        # 4. the constrained steps
        if method == ST:
            Lk = np.asarray(bone_len, np.float32).astype(np.float64).reshape(N, K)
            for s in range(n_steps):
                bk = b.reshape(N, K, 3)
                start = np.sqrt((bk[..., 0] * bk[..., 0] + bk[..., 1] * bk[..., 1]) + bk[..., 2] * bk[..., 2])
                target = (start * float(n_steps - s - 1) + Lk) / float(n_steps - s)
                rhs = (start * start - target * target) / 4.0
                S = np.zeros((N, K, K))
                for k in range(K):
                    for l in range(K):
                        acc = np.zeros(N)
                        for a in range(3):
                            t = np.zeros(N)
                            for c in range(3):
                                t = t + Inv[:, 3 * k + a, 3 * l + c] * bk[:, l, c]
                            acc = acc + bk[:, k, a] * t
                        S[:, k, l] = acc
                LS_, okS = chol(S)
                y = np.zeros((N, K))
                for i in range(K):
                    sacc = rhs[:, i].copy()
                    for k in range(i):
                        sacc = sacc - LS_[:, i, k] * y[:, k]
                    y[:, i] = sacc / LS_[:, i, i]
                lam = np.zeros((N, K))
                for i in range(K - 1, -1, -1):
                    sacc = y[:, i].copy()
                    for k in range(i + 1, K):
                        sacc = sacc - LS_[:, k, i] * lam[:, k]
                    lam[:, i] = sacc / LS_[:, i, i]
                d = np.repeat(2.0 * lam, 3, axis=1)
                acc = np.zeros((N, n, n))
                for j in range(n):
                    acc = acc + (Inv[:, :, j, None] * d[:, j, None, None]) * Inv[:, None, j, :]
                Inv_new = _mirror(Inv - acc)
                b_new = _matvec(Inv_new, beta)
                live = status == 0
                status = np.where(live & ~okS, 2, status).astype(np.int32)
                go = live & okS
                Inv = np.where(go[:, None, None], Inv_new, Inv)
                b = np.where(go[:, None], b_new, b)
        # 5. root, joints
        q = np.zeros((N, 3))
        for k in range(K):
            for c in range(3):
                q = q + C[:, k, :, c] * b[:, 3 * k + c, None]
        x0 = _matvec(Tinv, mu - q)
        X = np.zeros((N, J, 3))
        for i in range(J):
            x = x0.copy()
            for k in range(1, J):
                if k in anc[i]:
                    x = x + b[:, 3 * (k - 1):3 * k]
            X[:, i] = x
        X = np.where((status == 1)[:, None, None], 0.0, X)
        return (X.astype(np.float32), status, X) if full else (X.astype(np.float32), status)


def _gather(ud, conf, Pm, bone_len, per_person, b_idx, q_idx, p_idx, J):
    B, V = ud.shape[:2]
    udq = ud.reshape(B, V, -1, J, 2)
    sel_ud = np.stack([udq[b, :, q] for b, q in zip(b_idx, q_idx)]) if len(b_idx) else np.zeros((0, V, J, 2), np.float32)
    sel_cf = None
    if conf is not None:
        cq = conf.reshape(B, V, -1, J)
        sel_cf = np.stack([cq[b, :, q] for b, q in zip(b_idx, q_idx)])
    sel_P = Pm[b_idx]
    if bone_len is None:
        sel_L = None
    elif per_person:
        sel_L = np.stack([bone_len[b, p] for b, p in zip(b_idx, p_idx)])
    else:
        sel_L = np.broadcast_to(np.asarray(bone_len).reshape(1, J - 1), (len(b_idx), J - 1))
    return sel_ud, sel_cf, sel_P, sel_L


def _run(ud, conf, Pm, parent, bone_len, persons, P, method, n_steps):
    """persons: list of (b, p, q) that are computed; every other (b, p) gets X = 0, status -1"""
    B, J = ud.shape[0], len(parent)
    X = np.zeros((B, P, J, 3), np.float32)
    status = np.full((B, P), -1, np.int32)
    if persons:
        b_idx, p_idx, q_idx = (np.array(t) for t in zip(*persons))
        per_person = bone_len is not None and np.asarray(bone_len).ndim == 3
        args = _gather(np.asarray(ud), None if conf is None else np.asarray(conf), np.asarray(Pm), bone_len, per_person, b_idx,
                       q_idx, p_idx, J)
        x, s = solve(args[0], args[1], args[2], parent, args[3], method, n_steps)
        X[b_idx, p_idx], status[b_idx, p_idx] = x, s
    return X, status


def dense(ud, conf, Pm, parent, bone_len, valid=None, method="ST", n_steps=1):
    """ud (B, V, NQ*J, 2), conf (B, V, NQ*J) or None, Pm (B, V, 3, 4), valid (B, NQ) or None -> X (B, NQ, J, 3), status (B, NQ)"""
    B, J = ud.shape[0], len(parent)
    NQ = ud.shape[2] // J
    persons = [(b, q, q) for b in range(B) for q in range(NQ) if valid is None or valid[b, q] != 0]
    return _run(ud, conf, Pm, parent, bone_len, persons, NQ, method, n_steps)


def by_rows(ud, conf, Pm, parent, bone_len, rows, count=None, method="ST", n_steps=1):
    """rows (B, R) int32 query indices, count (B, 2) or None: person (b, r) is query rows[b, r] for r < count[b, 0]"""
    B, J = ud.shape[0], len(parent)
    NQ = ud.shape[2] // J
    R = rows.shape[1]
    persons = []
    for b in range(B):
        live = R if count is None else min(max(int(count[b, 0]), 0), R)
        persons += [(b, r, int(rows[b, r])) for r in range(live) if 0 <= int(rows[b, r]) < NQ]
    return _run(ud, conf, Pm, parent, bone_len, persons, R, method, n_steps)
