"""NumPy restatements of the arith="fast" operators of lbm_device.hpp.  TEST INFRASTRUCTURE ONLY.

The device's fast forms are the same operators as the strict ones, with the sums factored and fused multiply-adds: no
reference line restates them.  Written here operation for operation as lbm_device.hpp spells them (a fused multiply-add
is a*b + c), so that, evaluated in long double, they can be compared with the oracle's dense operator
(oracle.lbm_numpy.CavityOracle.collide): the algebra must agree to long-double rounding on any state, the lid row included.

  mrt_fast      collide<T, C_MRT_FAST>            the factored MRT operator
  srt_trt_fast  equ_collide<T, C_SRT/TRT_FAST>    SRT / TRT with the equilibrium never formed
  history_fast  equ_collide, TURB                 the closure's history sum_k cx cy feq_k = rho ux uy
"""


def mrt_fast(f, rho, w_e, w_eps, w_q, w_nu, meq_density="rho"):
    """f[9]: populations of the cells; rho: the density macros() gives them (on the lid row the overridden
    rho_l = f0 + f1 + f3 + 2 (f2 + f5 + f6)).  meq_density="r" builds m_eq[1], m_eq[2] from the plain population sum
    instead, as the factored form did before it was fixed; tests keep it to show that the check sees the difference."""
    R = type(f[0].flat[0])
    a13, d13, a24, d24 = f[1] + f[3], f[1] - f[3], f[2] + f[4], f[2] - f[4]
    a57, d57, a68, d68 = f[5] + f[7], f[5] - f[7], f[6] + f[8], f[6] - f[8]
    sa, sd, dm, dp = a13 + a24, a57 + a68, d57 - d68, d57 + d68
    r = (f[0] + sa) + sd                                      # m0
    rq = rho if meq_density == "rho" else r                   # the density of m_eq[1], m_eq[2]
    jx, jy = d13 + dm, d24 + dp
    f04 = R(4) * f[0]
    e = (R(2) * sd + -sa) - f04
    eps = R(-2) * sa + (f04 + sd)
    qx, qy = R(-2) * d13 + dm, R(-2) * d24 + dp
    pxx, pxy = a13 - a24, a57 - a68
    jx2, jy2 = jx * jx, jy * jy
    j23 = R(3) * (jx2 + jy2)
    e = -w_e * (e - (R(-2) * rq + j23)) + e
    eps = -w_eps * (eps - (R(9) * (jx2 * jy2) + (rq - j23))) + eps
    qx = -w_q * (qx - jx * (R(3) * jx2 + R(-1))) + qx
    qy = -w_q * (qy - jy * (R(3) * jy2 + R(-1))) + qy
    pxx = -w_nu * (pxx - (jx2 - jy2)) + pxx
    pxy = -w_nu * (-jx * jy + pxy) + pxy
    a9, a36, a18, a6, a12, a4 = R(1) / 9, R(1) / 36, R(1) / 18, R(1) / 6, R(1) / 12, R(1) / 4
    r9 = a9 * r
    out = [None] * 9
    out[0] = a9 * ((r - e) + eps)
    A = -a18 * eps + (-a36 * e + r9)
    D = a36 * eps + (a18 * e + r9)
    Ap, Am, Dp, Dm = a4 * pxx + A, -a4 * pxx + A, a4 * pxy + D, -a4 * pxy + D
    bx, by = a6 * (jx - qx), a6 * (jy - qy)
    X, Y = a12 * qx + a6 * jx, a12 * qy + a6 * jy
    XpY, XmY = X + Y, X - Y
    out[1], out[3] = Ap + bx, Ap - bx
    out[2], out[4] = Am + by, Am - by
    out[5], out[7] = Dp + XpY, Dp - XpY
    out[8], out[6] = Dm + XmY, Dm - XmY
    return out


def srt_trt_fast(coll, g, rho, ux, uy, w_nu, w_m=None):
    """The fused SRT / TRT operators: feq_a/b = rho t (B + 4.5 cu^2 +- 3 cu), B = 1 - 1.5 u^2, never formed."""
    R = type(g[0].flat[0])
    base = R(-1.5) * (uy * uy + ux * ux) + R(1)
    out = [None] * 9
    if coll == "SRT":
        orho, c1 = w_nu * rho, R(1) - w_nu
        r1, r5 = (R(1) / 9) * orho, (R(1) / 36) * orho
        out[0] = ((R(4) / 9) * orho) * base + c1 * g[0]

        def pair(cu, rw, a, b):
            e, o = (R(4.5) * cu) * cu + base, R(3) * cu
            out[a] = rw * (e + o) + c1 * g[a]
            out[b] = rw * (e - o) + c1 * g[b]
        pair(ux, r1, 1, 3); pair(uy, r1, 2, 4); pair(ux + uy, r5, 5, 7); pair(ux - uy, r5, 8, 6)
        return out
    assert coll == "TRT"
    orho, c1 = w_nu * rho, R(1) - w_nu
    out[0] = ((R(4) / 9) * orho) * base + c1 * g[0]
    r1, r5 = (R(1) / 9) * orho, (R(1) / 36) * orho
    mrho, hp, hm = w_m * rho, R(0.5) * w_nu, R(0.5) * w_m
    m1, m5 = (R(1) / 9) * mrho, (R(1) / 36) * mrho

    def pair(cu, rp, rm, a, b):
        e, o = (R(4.5) * cu) * cu + base, R(3) * cu
        P = -rp * e + hp * (g[a] + g[b])
        M = -rm * o + hm * (g[a] - g[b])
        out[a] = (g[a] - P) - M
        out[b] = (g[b] - P) + M
    pair(ux, r1, m1, 1, 3); pair(uy, r1, m1, 2, 4); pair(ux + uy, r5, m5, 5, 7); pair(ux - uy, r5, m5, 8, 6)
    return out


def history_fast(rho, ux, uy):
    return rho * (ux * uy)
