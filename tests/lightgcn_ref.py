"""Float64 references of the graph propagation and of the LightGCN train step (tests/test_lightgcn_cpu.py,
tests/test_gpu_lightgcn.py).  Two independent forms: the propagation over the two CSRs in NumPy (`propagate`), whose backward pass
is the same propagation applied to the gradient tables (`grads_csr`), and a DENSE A~ of size (NU + NI)^2 under torch float64
autograd (`loss_dense`, `train`), which knows nothing of that symmetry.  The CPU test holds the two to 1e-12."""
import numpy as np

U32 = 2.0 ** -24          # unit roundoff of float32


def csr_pair(users, items, nu, ni):
    """records -> ((ptr, cols) user -> items, (ptr, cols) item -> users): sorted, distinct, int64 / int32"""
    def one(r, c, nr, nc):
        key = np.unique(np.asarray(r, np.int64) * nc + np.asarray(c, np.int64))
        ptr = np.zeros(nr + 1, np.int64)
        np.cumsum(np.bincount(key // nc, minlength=nr), out=ptr[1:])
        return ptr, (key % nc).astype(np.int32)
    return one(users, items, nu, ni), one(items, users, ni, nu)


def records_of(ptr, cols):
    rec = np.zeros(cols.size, dtype=[("user_id", np.int32), ("item_id", np.int32)])
    rec["user_id"] = np.repeat(np.arange(ptr.size - 1), np.diff(ptr)); rec["item_id"] = cols
    return rec


def scales(ptr):
    """1 / sqrt(degree) in float32 as the library forms it on the host, exact 0 for degree 0"""
    deg = np.diff(ptr).astype(np.float32)
    out = np.zeros(deg.shape, np.float32)
    out[deg > 0] = np.float32(1) / np.sqrt(deg[deg > 0])
    return out


def unit(n):
    return np.ones(n, np.float32)


def half_layer(X, ptr, cols, rs, cs, dtype=np.float64, reverse=False):
    """y[r] = rs[r] * sum_e cs[cols[e]] * X[cols[e]] in `dtype`; float32: the terms are added one after the other in CSR order
    (reverse: in the opposite order)"""
    X = np.asarray(X, dtype); rs = np.asarray(rs, dtype); cs = np.asarray(cs, dtype)
    R = ptr.size - 1
    out = np.zeros((R, X.shape[1]), dtype)
    if dtype == np.float64:
        np.add.at(out, np.repeat(np.arange(R), np.diff(ptr)), cs[cols][:, None] * X[cols])
        return rs[:, None] * out
    n = np.diff(ptr)
    for j in range(int(n.max()) if n.size else 0):          # the j-th term of every row that has one (sequential per row)
        live = np.nonzero(n > j)[0]
        e = (ptr[live + 1] - 1 - j) if reverse else (ptr[live] + j)
        out[live] = out[live] + cs[cols[e]][:, None] * X[cols[e]]
    return rs[:, None] * out


def propagate(U, V, by_user, by_item, su, sv, alphas, dtype=np.float64, reverse=False):
    """E_f = sum_k alphas[k] A~^k [U ; V] -> (Uf, Vf) in `dtype`"""
    al = np.asarray(alphas, dtype)
    cu, cv = np.asarray(U, dtype), np.asarray(V, dtype)
    fu, fv = al[0] * cu, al[0] * cv
    for k in range(1, al.size):
        nu = half_layer(cv, *by_user, su, sv, dtype, reverse)
        nv = half_layer(cu, *by_item, sv, su, dtype, reverse)
        fu = fu + al[k] * nu; fv = fv + al[k] * nv
        cu, cv = nu, nv
    return fu, fv


def bound(U, V, by_user, by_item, su, sv, alphas):
    """the worst-case elementwise bound of a float32 evaluation: L (n_max + 8) u P(|U|, |V|), P the same propagation in float64
    on the absolute tables with the absolute layer weights"""
    L = len(alphas) - 1
    n_max = int(max(np.diff(by_user[0]).max(), np.diff(by_item[0]).max()))
    pu, pv = propagate(np.abs(U), np.abs(V), by_user, by_item, su, sv, np.abs(np.asarray(alphas, np.float64)))
    f = L * (n_max + 8) * U32
    return f * pu, f * pv, n_max


def dense_A(by_user, su, sv, nu, ni):
    """A~ as a float64 matrix over [users ; items]"""
    A = np.zeros((nu + ni, nu + ni))
    ptr, cols = by_user
    r = np.repeat(np.arange(nu), np.diff(ptr))
    w = np.asarray(su, np.float64)[r] * np.asarray(sv, np.float64)[cols]
    A[r, nu + cols] = w
    A[nu + cols, r] = w
    return A


def propagate_dense(A, U, V, alphas):
    E = np.concatenate([np.asarray(U, np.float64), np.asarray(V, np.float64)])
    F = alphas[0] * E
    for k in range(1, len(alphas)):
        E = A @ E
        F = F + alphas[k] * E
    return F[:U.shape[0]], F[U.shape[0]:]


def loss_dense(A, U, V, alphas, uid, pid, nid, l2_reg):
    """torch float64 autograd through the dense A~ -> (loss, l2, dJ/dU, dJ/dV), J = loss + l2"""
    import torch
    At = torch.from_numpy(np.asarray(A, np.float64))
    Ut = torch.tensor(np.asarray(U, np.float64), requires_grad=True)
    Vt = torch.tensor(np.asarray(V, np.float64), requires_grad=True)
    E = torch.cat([Ut, Vt])
    F = alphas[0] * E
    for k in range(1, len(alphas)):
        E = At @ E
        F = F + float(alphas[k]) * E
    nu = Ut.shape[0]
    u, p, n = (torch.from_numpy(np.asarray(x, np.int64)) for x in (uid, pid, nid))
    x = (F[u] * (F[nu + p] - F[nu + n])).sum(1)
    loss = torch.nn.functional.softplus(-x).mean()
    l2 = float(l2_reg) / len(uid) * 0.5 * ((Ut[u] ** 2).sum() + (Vt[p] ** 2).sum() + (Vt[n] ** 2).sum())
    (loss + l2).backward()
    return float(loss.detach()), float(l2.detach()), Ut.grad.numpy().copy(), Vt.grad.numpy().copy()


def grads_csr(U, V, by_user, by_item, su, sv, alphas, uid, pid, nid, l2_reg):
    """the same by hand over the CSRs: the gradient w.r.t. the propagated rows, propagated by the SAME operator, plus the l2 term
    of the layer-0 rows per occurrence -> (loss, l2, dJ/dU, dJ/dV)"""
    U = np.asarray(U, np.float64); V = np.asarray(V, np.float64)
    B = len(uid)
    fu, fv = propagate(U, V, by_user, by_item, su, sv, alphas)
    x = (fu[uid] * (fv[pid] - fv[nid])).sum(1)
    loss = float(np.mean(np.logaddexp(0.0, -x)))
    g = -1.0 / (1.0 + np.exp(x)) / B
    GU = np.zeros_like(U); GV = np.zeros_like(V)
    np.add.at(GU, uid, g[:, None] * (fv[pid] - fv[nid]))
    np.add.at(GV, pid, g[:, None] * fu[uid])
    np.add.at(GV, nid, -g[:, None] * fu[uid])
    gu, gv = propagate(GU, GV, by_user, by_item, su, sv, alphas)
    c = float(l2_reg) / B
    np.add.at(gu, uid, c * U[uid]); np.add.at(gv, pid, c * V[pid]); np.add.at(gv, nid, c * V[nid])
    l2 = c * 0.5 * float((U[uid] ** 2).sum() + (V[pid] ** 2).sum() + (V[nid] ** 2).sum())
    return loss, l2, gu, gv


def bpr_dense_grads(U, V, uid, pid, nid):
    """the bias-free BPR step's objective on the RAW rows, loss only (rt.pairwise_step("bpr", ..., bias=None, no_l2=True))"""
    U = np.asarray(U, np.float64); V = np.asarray(V, np.float64)
    x = (U[uid] * (V[pid] - V[nid])).sum(1)
    g = -1.0 / (1.0 + np.exp(x)) / len(uid)
    GU = np.zeros_like(U); GV = np.zeros_like(V)
    np.add.at(GU, uid, g[:, None] * (V[pid] - V[nid]))
    np.add.at(GV, pid, g[:, None] * U[uid])
    np.add.at(GV, nid, -g[:, None] * U[uid])
    return GU, GV


class DenseOpt:
    """the Keras dense rules in float64, one state per table name"""

    def __init__(self, kind, lr, momentum=0.0, nesterov=False, initial_accumulator_value=0.1, epsilon=1e-7, beta_1=0.9, beta_2=0.999):
        self.kind, self.lr, self.mom, self.nesterov = kind, lr, momentum, nesterov
        self.acc0, self.eps, self.b1, self.b2 = initial_accumulator_value, epsilon, beta_1, beta_2
        self.t, self.s = 0, {}

    def advance(self):
        self.t += 1

    def apply(self, name, w, g):
        if self.kind == "sgd":
            return w - self.lr * g
        if self.kind == "momentum":
            a = self.s.get(name, np.zeros_like(w)) * self.mom - self.lr * g
            self.s[name] = a
            return w + (self.mom * a - self.lr * g if self.nesterov else a)
        if self.kind == "adagrad":
            a = self.s.get(name, np.full_like(w, self.acc0)) + g * g
            self.s[name] = a
            return w - self.lr * g / (np.sqrt(a) + self.eps)
        m, v = self.s.get(name, (np.zeros_like(w), np.zeros_like(w)))
        m = self.b1 * m + (1 - self.b1) * g; v = self.b2 * v + (1 - self.b2) * g * g
        self.s[name] = (m, v)
        lr_t = self.lr * np.sqrt(1 - self.b2 ** self.t) / (1 - self.b1 ** self.t)
        return w - lr_t * m / (np.sqrt(v) + self.eps)


def train(A, U, V, alphas, opt, batches, l2_reg, train_tables=("user", "item")):
    """`batches`: a list of ("graph", uid, pid, nid) / ("bpr", uid, pid, nid) steps on one optimizer -> (U, V, [(loss, l2)])
    in float64 (losses of the graph steps only)"""
    U = np.asarray(U, np.float64).copy(); V = np.asarray(V, np.float64).copy()
    out = []
    for kind, uid, pid, nid in batches:
        if kind == "graph":
            loss, l2, gu, gv = loss_dense(A, U, V, alphas, uid, pid, nid, l2_reg)
            out.append((loss, l2))
            names = train_tables
        else:
            gu, gv = bpr_dense_grads(U, V, uid, pid, nid)
            names = ("user", "item")
        opt.advance()
        if "user" in names:
            U = opt.apply("user", U, gu)
        if "item" in names:
            V = opt.apply("item", V, gv)
    return U, V, out
