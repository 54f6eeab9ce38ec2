"""An independent float64 restatement of Brox optical flow -- TEST INFRASTRUCTURE.

Written from the publication's equations (Brox, Bruhn, Papenberg, Weickert, ECCV 2004, eq. 9-13 in the incremental form of
IPOL's "Robust Optical Flow Estimation", section 3), not from the float32 oracle: every inner step BUILDS the linear system
``A x = b`` of the Euler-Lagrange equations with frozen nonlinearities as a sparse matrix over ``x = (du, dv)`` and applies
successive over-relaxation from the matrix (a triangular solve in the red-black order), where the oracle and the kernels
update pixels from nine coefficients.  Pyramid, derivatives and upsampling are restated in float64 as well; only the
Gaussian taps of S1 are the specification's float32 numbers.
"""
import numpy as np
import scipy.sparse as sp
from scipy.sparse.linalg import spsolve_triangular

from oracle import tvl1_oracle


def sample(img, px, py):
    h, w = img.shape
    x = np.clip(px, 0.0, w - 1.0)
    y = np.clip(py, 0.0, h - 1.0)
    x0, y0 = np.floor(x).astype(int), np.floor(y).astype(int)
    x1, y1 = np.minimum(x0 + 1, w - 1), np.minimum(y0 + 1, h - 1)
    ax, ay = x - x0, y - y0
    return (1 - ay) * ((1 - ax) * img[y0, x0] + ax * img[y0, x1]) + ay * ((1 - ax) * img[y1, x0] + ax * img[y1, x1])


def grad(a):
    p = np.pad(a, 1, mode="edge")
    return 0.5 * (p[1:-1, 2:] - p[1:-1, :-2]), 0.5 * (p[2:, 1:-1] - p[:-2, 1:-1])


def zoom_out(img, step, ow, oh):
    R, taps = tvl1_oracle.zoom_taps(step)
    taps = taps.astype(np.float64)
    h, w = img.shape
    p = np.pad(img, ((0, 0), (R, R)), mode="edge")
    t = sum(taps[k] * p[:, k:k + w] for k in range(2 * R + 1))
    p = np.pad(t, ((R, R), (0, 0)), mode="edge")
    t = sum(taps[k] * p[k:k + h, :] for k in range(2 * R + 1))
    fx, fy = np.float32(w) / np.float32(ow), np.float32(h) / np.float32(oh)  # (the specification's float32 ratios)
    return sample(t, np.arange(ow)[None, :] * float(fx) + np.zeros((oh, 1)), np.arange(oh)[:, None] * float(fy) + np.zeros((1, ow)))


def upsample(uc, fw, fh, step):
    ch, cw = uc.shape
    rx, ry = float(np.float32(cw) / np.float32(fw)), float(np.float32(ch) / np.float32(fh))
    inv = float(np.float32(1.0) / np.float32(step))
    return sample(uc, np.arange(fw)[None, :] * rx + np.zeros((fh, 1)), np.arange(fh)[:, None] * ry + np.zeros((1, fw))) * inv


def system(f, u, v, du, dv, p):
    """The linear system of one inner step, nonlinearities frozen at (du, dv): sparse symmetric A [2N,2N] and b [2N] over
    x = (du in raster order, dv in raster order)."""
    h, w = u.shape
    N = h * w
    e2 = float(p["epsilon"]) ** 2
    Ix, Iy, Ixx, Ixy, Iyy, Iz, Ixz, Iyz = (f[k] for k in ("Ix", "Iy", "Ixx", "Ixy", "Iyy", "Iz", "Ixz", "Iyz"))
    psiD = 1.0 / np.sqrt((Iz + Ix * du + Iy * dv) ** 2 + e2)
    psiG = p["gamma"] / np.sqrt((Ixz + Ixx * du + Ixy * dv) ** 2 + (Iyz + Ixy * du + Iyy * dv) ** 2 + e2)
    ux, uy = grad(u + du)
    vx, vy = grad(v + dv)
    psiS = p["alpha"] / np.sqrt(ux ** 2 + uy ** 2 + vx ** 2 + vy ** 2 + e2)
    idx = np.arange(N).reshape(h, w)
    # the weighted graph Laplacian of the four-neighbourhood: edge weight = mean of PsiS at its two ends
    ei = np.concatenate([idx[:, :-1].ravel(), idx[:-1, :].ravel()])
    ej = np.concatenate([idx[:, 1:].ravel(), idx[1:, :].ravel()])
    ew = np.concatenate([0.5 * (psiS[:, :-1] + psiS[:, 1:]).ravel(), 0.5 * (psiS[:-1, :] + psiS[1:, :]).ravel()])
    Wm = sp.coo_matrix((np.concatenate([ew, ew]), (np.concatenate([ei, ej]), np.concatenate([ej, ei]))), shape=(N, N)).tocsr()
    Lap = sp.diags(np.asarray(Wm.sum(axis=1)).ravel()) - Wm
    a11 = (psiD * Ix * Ix + psiG * (Ixx * Ixx + Ixy * Ixy)).ravel()
    a12 = (psiD * Ix * Iy + psiG * (Ixx * Ixy + Ixy * Iyy)).ravel()
    a22 = (psiD * Iy * Iy + psiG * (Ixy * Ixy + Iyy * Iyy)).ravel()
    A = sp.bmat([[sp.diags(a11) + Lap, sp.diags(a12)], [sp.diags(a12), sp.diags(a22) + Lap]]).tocsr()
    b = np.concatenate([-(psiD * Ix * Iz + psiG * (Ixx * Ixz + Ixy * Iyz)).ravel() - Lap @ u.ravel(),
                        -(psiD * Iy * Iz + psiG * (Ixy * Ixz + Iyy * Iyz)).ravel() - Lap @ v.ravel()])
    return A, b


def redblack_order(h, w):
    """The unknowns in the order S61 visits them: per pixel du then dv, pixels with (x + y) even first."""
    N = h * w
    par = (np.add.outer(np.arange(h), np.arange(w)) & 1).ravel()
    pix = np.concatenate([np.flatnonzero(par == 0), np.flatnonzero(par == 1)])
    return np.stack([pix, pix + N], axis=1).ravel()


def sor_sweep(A, b, x, omega, order):
    """One SOR sweep over the unknowns in `order`, from the matrix: (D/omega + L) x' = b - (U + (1 - 1/omega) D) x."""
    Ap = A[order][:, order].tocsr()
    D = sp.diags(Ap.diagonal())
    Lo, Up = sp.tril(Ap, -1), sp.triu(Ap, 1)
    xp = spsolve_triangular((D / omega + Lo).tocsr(), b[order] - (Up + (1.0 - 1.0 / omega) * D) @ x[order], lower=True)
    out = np.empty_like(x)
    out[order] = xp
    return out


def energy(A, b, x):
    return 0.5 * x @ (A @ x) - b @ x


def warp(d0, d1, u, v):
    h, w = u.shape
    px, py = np.arange(w)[None, :] + u, np.arange(h)[:, None] + v
    I1w, Ix, Iy, Ixx, Ixy, Iyy = (sample(f, px, py) for f in d1)
    return dict(Ix=Ix, Iy=Iy, Ixx=Ixx, Ixy=Ixy, Iyy=Iyy, Iz=I1w - d0[0], Ixz=Ix - d0[1], Iyz=Iy - d0[2])


def derivatives(img):
    ix, iy = grad(img)
    return img, ix, iy, grad(ix)[0], grad(iy)[0], grad(iy)[1]


def flow_pair(i0, i1, p):
    """two gray frames [H,W] in [0,255] -> flow [2,H,W] float64"""
    h, w = np.asarray(i0).shape
    sizes = tvl1_oracle.pyramid_sizes(w, h, p["nscales"], p["scale_step"])
    pyr = []
    for img in (i0, i1):
        lv = [np.asarray(img, dtype=np.float64) / 255.0]
        for (lw, lh) in sizes[1:]:
            lv.append(zoom_out(lv[-1], p["scale_step"], lw, lh))
        pyr.append(lv)
    u = np.zeros(pyr[0][-1].shape)
    v = np.zeros_like(u)
    for s in range(len(sizes) - 1, -1, -1):
        lh, lw = u.shape
        order = redblack_order(lh, lw)
        d0, d1 = derivatives(pyr[0][s]), derivatives(pyr[1][s])
        for _ in range(p["warps"]):
            f = warp(d0, d1, u, v)
            x = np.zeros(2 * lh * lw)
            for _ in range(p["inner_iters"]):
                A, b = system(f, u, v, x[:lh * lw].reshape(lh, lw), x[lh * lw:].reshape(lh, lw), p)
                for _ in range(p["solver_iters"]):
                    x = sor_sweep(A, b, x, p["omega"], order)
            u, v = u + x[:lh * lw].reshape(lh, lw), v + x[lh * lw:].reshape(lh, lw)
        if s > 0:
            fw, fh = sizes[s - 1]
            u, v = upsample(u, fw, fh, p["scale_step"]), upsample(v, fw, fh, p["scale_step"])
    return np.stack([u, v])
