"""A second, independent restatement of the step's arithmetic, against which the ORACLE is checked.

`oracle/step.c` follows the reference routine by routine (lists, f32, the reference's loop order).  This file states the same
physics once more from the reference's equations as DENSE f64 linear algebra in numpy -- n x n kernel matrices, the divergence and the
pressure acceleration as matrices, a_ii as the DIAGONAL of their product instead of the reference's closed form -- for a free block of
fluid far from every wall (no boundary terms), one IISPH or HybridDFSPH step with a fixed number of Jacobi iterations.  A slip in the oracle's
indexing, signs, operator discretisation, iteration count or update order shows here; a slip in the closed form of a_ii shows
against the operator it is supposed to be the diagonal of.  (What neither restatement can catch is a misreading of the physics
shared by both -- they have the same reader.)

Equations (reference file:line):
  h_i = 1.9 sqrt(m_i / (rho_0 pi))                                   simulation.rs:371-380, sph_kernels.rs:203-206
  j in N(i)  <=>  |x_ij| < 2 h_ij,  h_ij = (h_i + h_j) / 2           neighborhood_search.rs:143-146 (i itself included)
  W(r, h) = 10 / (7 pi h^2) w(r / 2h), grad W = 10 / (7 pi h^2) w'(q) / (2h) x / r, zero for q <= 1e-5     sph_kernels.rs:23-71
  rho_i = sum_j m_j W_ij                                             simulation.rs:1007-1028
  v* = v + dt (g + nu sum_j 8 m_j / rho_ij (x_ij . v_ij) / (|x_ij|^2 + 0.01 h_ij^2) grad W_ij over the pairs with x_ij . v_ij < 0)
                                                                     simulation.rs:931-1005, 1051-1077 (ApproxLaplace)
  div(Q)_i = sum_j m_j / rho_i (Q_j - Q_i) . grad W_ij               simulation.rs:1552-1593 (ConsistentSimpleGradient)
  s_i = -(rho_0 - rho_i) / (rho_i dt^2) - div(v*)_i / dt             simulation.rs:1712-1749
  a^p_i = -sum_j m_j (p_i / rho_i^2 + p_j / rho_j^2) grad W_ij       simulation.rs:1780-1808
  p <- max(0, p + omega (s - div(a^p[p])) / a_ii), |a_ii| < 1e-3 -> 0, max_iters + 1 times from p = 0       simulation.rs:1207-1322, 1378-1480
  a^p from the final p;  v <- v* + dt a^p;  x <- x + dt v           simulation.rs:1499-1509, 2427-2445
  HybridDFSPH: divergence solve (s = -div(v) / dt), v += dt a^p, forces before or after it, density solve (full source term or
  its density part), x += dt v + dt^2 a^p, v += dt a^p min(dt factor, 1)                                  simulation.rs:2502-2670
"""
import numpy as np
import pytest

from adaptive_sph_amd import ffi, scene as sc
from adaptive_sph_amd.workloads import dam_break_params
from tests.oracle_harness import load_oracle


def boundary_terms(pos, h, planes, penalty_term, lam, dlam):
    """sum of lambda and of grad lambda per particle over the planes it touches (boundary_winchenbach2020.rs:58-152): d = sdf / (2 h_i),
    lambda(d) and its derivative from the closed forms (plane_numerics.rs; the oracle's f64 functions, pinned to the reference's
    Maxima values in test_oracle_golden.py), the four penalty terms (:84-128: None 1, Linear 1 - d, Quadratic1 with its knee at d = -1,
    Quadratic2 with its knee at d = -0.5; all but Linear are 1 in front of the wall), gradient along the plane's normal"""
    n = len(h)
    ls, gl = np.zeros(n), np.zeros((n, 2))
    for (nx, ny, delta) in planes:
        sr = 2.0 * h
        dd = (nx * pos[:, 0] + ny * pos[:, 1] + delta) / sr
        for i in np.nonzero(dd < 1.0)[0]:
            d = dd[i]
            if penalty_term == "None":
                pen, dpen = 1.0, 0.0
            elif penalty_term == "Linear":
                pen, dpen = 1.0 - d, -1.0
            elif penalty_term == "Quadratic1":
                pen = 1.0 if d > 0 else (0.5 * d * d + 1.0 if d > -1.0 else 0.5 - d)
                dpen = 0.0 if d > 0 else (d if d > -1.0 else -1.0)
            else:
                assert penalty_term == "Quadratic2"
                pen = 1.0 if d > 0 else (d * d + 1.0 if d > -0.5 else 0.75 - d)
                dpen = 0.0 if d > 0 else (2.0 * d if d > -0.5 else -1.0)
            la, dla = (1.0, 0.0) if d <= -1.0 else (lam(d), dlam(d))
            ls[i] += la * pen
            gl[i] += np.array([nx, ny]) / sr[i] * (dpen * la + pen * dla)
    return ls, gl


def dense_step(pos, mass, vel, P, dt, n_iterations, planes=(), lam=None, dlam=None, cutoff=1.0e-5, nb=None):
    """one step (IISPH or HybridDFSPH, viscosity ApproxLaplace, plane boundaries, the three operator discretisations) as
    dense f64 linear algebra; every solve runs `n_iterations` Jacobi iterations from p = 0.  `cutoff`: the reference's q below which
    grad W is zero (sph_kernels.rs:57-59); None: no cut-off, the gradient of every pair with r > 0 (tests/test_gpu_branch_points.py).
    `nb`: the neighbour relation (n x n bool) where f64 cannot restate it -- pairs within an f32 rounding of the support's edge, where W
    and its gradient vanish and only the count tells"""
    pos, mass, vel = pos.astype(np.float64), mass.astype(np.float64), vel.astype(np.float64)
    n = len(mass)
    rest_density, omega, disc = P.rest_density, P.jacobi_omega, P.operator_discretization
    h = 1.9 * np.sqrt(mass / rest_density / np.pi)
    d = pos[:, None, :] - pos[None, :, :]                     # x_ij
    r = np.sqrt((d ** 2).sum(2))
    hij = 0.5 * (h[:, None] + h[None, :])
    if nb is None:
        nb = r < 2.0 * hij
    q = r / (2.0 * hij)
    nf = 10.0 / (7.0 * np.pi * hij ** 2)
    w = np.where(q < 0.5, 6.0 * (q ** 3 - q ** 2) + 1.0, np.where(q < 1.0, 2.0 * (1.0 - q) ** 3, 0.0))
    dw = np.where(q < 0.5, 18.0 * q ** 2 - 12.0 * q, np.where(q < 1.0, -6.0 * (1.0 - q) ** 2, 0.0))
    W = nf * w * nb
    with np.errstate(invalid="ignore", divide="ignore"):
        unit = np.where((r > 0.0 if cutoff is None else q > cutoff)[:, :, None], d / r[:, :, None], 0.0)
    G = (nf * dw / (2.0 * hij) * nb)[:, :, None] * unit       # grad W_ij, n x n x 2
    lam_sum, lam_grad = boundary_terms(pos, h, planes, P.boundary_penalty_term, lam, dlam) if len(planes) else (np.zeros(n), np.zeros((n, 2)))
    rho = (mass[None, :] * W).sum(1) + lam_sum                # density_boundary_term = sum lambda (boundary_winchenbach2020.rs:154-163)
    counts = nb.sum(1)

    def non_pressure(v):    # simulation.rs:931-1005: viscosity over the approaching pairs (ApproxLaplace or WCSPH), gravity
        xv = (d * (v[:, None, :] - v[None, :, :])).sum(2)
        if P.viscosity_type == "WCSPH":   # -m_j Pi_ij grad W_ij, Pi_ij = -2 nu h_ij c / (rho_i + rho_j) (x . v) / (|x|^2 + 0.001 h_ij^2), c = 88
            pi_ab = -(2.0 * P.viscosity * hij * 88.0 / (rho[:, None] + rho[None, :])) * xv / (r ** 2 + 0.001 * hij ** 2)
            visc = ((-mass[None, :] * pi_ab * (xv < 0.0) * nb)[:, :, None] * G).sum(1)
        else:
            rho_ij = 0.5 * (rho[:, None] + rho[None, :])
            coeff = 2.0 * 4.0 * (mass[None, :] / rho_ij) * xv / (r ** 2 + 0.01 * hij ** 2)
            visc = P.viscosity * ((coeff * (xv < 0.0) * nb)[:, :, None] * G).sum(1)
        return visc + np.array([0.0, P.gravity])

    # the two operators as matrices per component c: div(Q) = sum_c D_c Q_c ;  a^p_c = A_c p
    D, A = [], []
    for c in range(2):
        # (Winchenbach2020 weighs the divergence's pairs with m_j / rho_j instead of m_j / rho_i, simulation.rs:1571-1580)
        Dc = (mass[None, :] / rho[None, :] if disc == "Winchenbach2020" else mass[None, :] / rho[:, None]) * G[:, :, c]
        Dc[np.arange(n), np.arange(n)] -= Dc.sum(1)           # -Q_i sum_j ... grad W_ij  (the j = i entry of G is zero)
        Ac = -mass[None, :] / rho[None, :] ** 2 * G[:, :, c]
        Ac[np.arange(n), np.arange(n)] += -(mass[None, :] * G[:, :, c]).sum(1) / rho ** 2
        # the walls: div += rho_0 / rho_i (0 - Q_i) . sum grad lambda ;  a^p += -rho_0 (p_i / rho_i^2 + 0) sum grad lambda
        # (boundary_winchenbach2020.rs:165-223, p_ib = 0 and rho_b = rho_0 in this discretisation)
        # (Winchenbach2020: the wall's divergence term without rho_0 / rho_i; ConsistentSymmetricGradient: p_ib = p_i)
        Dc[np.arange(n), np.arange(n)] += -(1.0 if disc == "Winchenbach2020" else rest_density / rho) * lam_grad[:, c]
        Ac[np.arange(n), np.arange(n)] += -rest_density * (1.0 / rho ** 2 + (1.0 / rest_density ** 2 if disc == "ConsistentSymmetricGradient" else 0.0)) * lam_grad[:, c]
        D.append(Dc)
        A.append(Ac)
    div = lambda Q: D[0] @ Q[:, 0] + D[1] @ Q[:, 1]          # noqa: E731
    accel = lambda p: np.stack([A[0] @ p, A[1] @ p], 1)       # noqa: E731
    aii = np.einsum("ij,ji->i", D[0], A[0]) + np.einsum("ij,ji->i", D[1], A[1])   # diag(D A)

    def solve(s):
        p = np.zeros(n)
        for _ in range(n_iterations):
            pn = p + omega * (s - div(accel(p))) / aii
            pn = np.where(np.abs(aii) < 10e-4, 0.0, pn)
            p = np.where(pn <= 0.0, 0.0, pn)
        return p, accel(p)

    out = dict(density=rho, neighbor_count=counts, aii=aii, lambda_sum=lam_sum, lambda_grad_sum=lam_grad)
    dens_part = -(rest_density - rho) / ((rest_density if disc == "Winchenbach2020" else rho) * dt * dt)   # simulation.rs:1661-1676, 1733-1745
    if P.pressure_solver_method == "IISPH":                                  # simulation.rs:2389-2446
        vstar = vel + dt * non_pressure(vel)
        s = dens_part - div(vstar) / dt
        p, ap = solve(s)
        v = vstar + dt * ap
        x = pos + dt * v
    elif P.pressure_solver_method == "IISPH2":                               # simulation.rs:2262-2387 (every particle's size class Optimal)
        Hi, Hij = 2.0 * h, 2.0 * hij
        qq = r / Hij
        wq = np.where(qq < 0.5, 6.0 * (qq ** 3 - qq ** 2) + 1.0, np.where(qq < 1.0, 2.0 * (1.0 - qq) ** 3, 0.0))
        dwq = np.where(qq < 0.5, 18.0 * qq ** 2 - 12.0 * qq, np.where(qq < 1.0, -6.0 * (1.0 - qq) ** 2, 0.0))
        cd = 40.0 / (7.0 * np.pi)
        dwdh = cd * -2.0 / Hij ** 3 * wq + cd / Hij ** 2 * dwq * (-r / Hij ** 2)
        om = np.minimum(2.5, np.maximum(1.0 + ((Hi / (3.0 * rho))[:, None] * (mass[None, :] * dwdh * nb)).sum(1), 0.125))
        out["omega"] = om
        vstar = vel + dt * non_pressure(vel)
        s = -(rest_density - rho) / (rest_density * dt * dt) - div(vstar) / (dt * om)
        p, _ = solve(s)
        p = p / np.sqrt(om)
        ap = accel(p)
        v = vstar + dt * ap
        x = pos + dt * v
    else:                                                                    # HybridDFSPH, simulation.rs:2502-2670
        before = P.hybrid_dfsph_non_pressure_accel_before_divergence_free
        v1 = vel + dt * non_pressure(vel) if before else vel
        p_div, ap_div = solve(-div(v1) / dt)
        out["pressure_div"] = p_div
        v2 = v1 + dt * ap_div
        if not before:
            v2 = v2 + dt * non_pressure(v2)
        s = dens_part if P.hybrid_dfsph_density_source_term == "OnlyDensity" else dens_part - div(v2) / dt
        p, ap = solve(s)
        x = pos + dt * v2 + dt * dt * ap
        v = v2 + dt * ap * min(dt * P.hybrid_dfsph_factor, 1.0)
    out.update(ppe_source_term=s, pressure=p, pressure_accel=ap, velocity=v, position=x, _nb=nb, _hij=hij)
    return out


def rel(a, b):
    s = np.abs(b).max()
    return np.abs(np.asarray(a, np.float64) - b).max() / (s if s > 0 else 1.0)


def _case(max_iters, solver="IISPH", wall=False, two_sizes=False, **kw):
    spacing = 0.03
    # (a block 12 % denser than rest: positive pressures inside, clamped ones along its rim -- both branches of the update;
    #  `wall`: the block sits in the lower left corner of the box, one spacing off two walls)
    origin = [-2.0 + 1.024 * spacing, -1.0 + 1.024 * spacing] if wall else [-0.3, -0.3]
    blocks = [sc.SceneFluidBlock(origin, [0.6001, 0.6001], spacing, 1.12, [0.0, 0.0])]
    if two_sizes:   # a second block of half the spacing (a quarter of the mass) against the first one's right side: h_ij = (h_i + h_j) / 2
        blocks.append(sc.SceneFluidBlock([origin[0] + 0.6 + 0.75 * spacing, origin[1]], [0.3001, 0.6001], spacing / 2, 1.12, [0.0, 0.0]))
    scn = sc.SceneConfig(sc.SceneBoundary("box", 4.0, 2.0), blocks)
    pos, mass, vel = sc.init_particles(scn)
    assert len(mass) == 20 * 20 + (20 * 40 if two_sizes else 0)
    rng = np.random.default_rng(5)
    pos = (pos + rng.uniform(-0.12, 0.12, pos.shape).astype(np.float32) * spacing).astype(np.float32)   # off the lattice: no symmetric cancellation
    vel = np.stack([0.3 * pos[:, 0] + 0.1 * pos[:, 1], -0.2 * pos[:, 1] + 0.05 * np.sin(9.0 * pos[:, 0])], 1).astype(np.float32)
    kw.setdefault("level_estimation_method", "None")
    P = dam_break_params(pressure_solver_method=solver, max_dt=1.0e-4, max_iters=max_iters, iisph_max_avg_density_error=0.0,
                         hybrid_dfsph_max_avg_density_error=0.0, hybrid_dfsph_max_avg_divergence_error=0.0, **kw)
    assert P.support_length_estimation == "FromMass"
    return scn, pos, mass, vel, P


def _compare(ctx, pos, mass, vel, P, max_iters, tol, planes=(), block=True, nb=None):
    """one step of `ctx` (oracle or product) against the dense restatement; `tol` scales the bars (1 = the oracle's f32 rounding).
    `block`: the scene is _case's block, whose rim clamps a tenth of the pressures (other scenes: both branches of the clamp taken);
    `nb`: dense_step's"""
    n = len(mass)
    L = load_oracle().lib
    ctx.upload(mass, pos, vel)
    st = ctx.step(P.to_ffi())
    assert st.dt == pytest.approx(1.0e-4, rel=1e-6)
    assert st.density_solver.iters == max_iters           # num_pressure_iters at the break: max_iters + 1 iterations ran
    ref = dense_step(pos, mass, vel, P, float(st.dt), max_iters + 1, planes, lambda d: float(L.oracle_lambda2(d)), lambda d: float(L.oracle_dlambda2(d)), nb=nb)
    if P.pressure_solver_method == "HybridDFSPH":
        assert st.div_solver.iters == max_iters
        assert (ref["pressure_div"] > 0).sum() > 0
    if len(planes):
        assert (ref["lambda_sum"] > 0).sum() > 30
        assert rel(ctx.download("lambda_sum"), ref["lambda_sum"]) <= 2e-6 * tol       # (the 10001-entry LUT against the closed form)
        assert rel(ctx.download("lambda_grad_sum"), ref["lambda_grad_sum"]) <= 2e-5 * tol
    else:
        assert np.abs(ctx.download("lambda_sum")).max() == 0.0     # far from every wall: no boundary terms in this scene
    assert np.array_equal(ctx.download("neighbor_count"), ref["neighbor_count"])
    assert ref["neighbor_count"].min() >= 4 and ref["neighbor_count"].max() <= 60
    assert np.abs(ref["aii"]).min() > 10e-4                                   # (nobody takes the singular branch)
    assert (ref["pressure"] > 0).sum() > n // 2 and (ref["pressure"] == 0).sum() > (n // 10 if block else 10)     # both branches of the clamp
    # measured with the oracle: 2e-7 (density), 6e-7 (a_ii: the closed form vs the diagonal of div . a^p), 3e-7 (source term),
    # 1.6e-6 (pressure after 1 and after 4 iterations), 1e-6 (a^p), 1e-6 / 4e-6 of the velocity / position CHANGE of the step
    assert rel(ctx.download("density"), ref["density"]) <= 2e-6 * tol
    assert rel(ctx.download("aii"), ref["aii"]) <= 5e-6 * tol
    assert rel(ctx.download("ppe_source_term"), ref["ppe_source_term"]) <= 5e-6 * tol
    assert rel(ctx.download("pressure"), ref["pressure"]) <= 1e-5 * tol
    assert rel(ctx.download("pressure_accel"), ref["pressure_accel"]) <= 1e-5 * tol
    dv_o, dv_r = ctx.download("velocity").astype(np.float64) - vel, ref["velocity"] - vel
    assert np.abs(dv_o - dv_r).max() <= 1e-5 * tol * np.abs(dv_r).max()
    dx_o, dx_r = ctx.download("position").astype(np.float64) - pos, ref["position"] - pos
    assert np.abs(dx_o - dx_r).max() <= 2e-5 * tol * np.abs(dx_r).max() + 1.2e-7


CASES = [("IISPH", dict(viscosity=0.0)), ("IISPH", dict()), ("HybridDFSPH", dict()), ("IISPH", dict(wall=True)), ("HybridDFSPH", dict(wall=True)),
         ("HybridDFSPH", dict(wall=True, two_sizes=True)),
         ("HybridDFSPH", dict(wall=True, operator_discretization="ConsistentSymmetricGradient")),
         ("HybridDFSPH", dict(wall=True, two_sizes=True, operator_discretization="Winchenbach2020")),
         ("IISPH", dict(wall=True, operator_discretization="Winchenbach2020")),
         ("IISPH", dict(viscosity_type="WCSPH", viscosity=0.05)),
         ("IISPH2", dict()), ("IISPH2", dict(wall=True)),
         ("HybridDFSPH", dict(hybrid_dfsph_density_source_term="OnlyDensity", hybrid_dfsph_non_pressure_accel_before_divergence_free=False))]


@pytest.mark.parametrize("solver,kw", CASES)
@pytest.mark.parametrize("max_iters", [0, 3])
def test_oracle_against_dense_f64_operators(max_iters, solver, kw):
    scn, pos, mass, vel, P = _case(max_iters, solver, **kw)
    planes = sc.boundary_planes(scn.boundary, P.init_boundary_handler)
    o = ffi.Context(load_oracle(), len(mass), planes)
    _compare(o, pos, mass, vel, P, max_iters, 1.0, planes if kw.get("wall") else ())


@pytest.mark.gpu
@pytest.mark.parametrize("solver,kw", CASES)
@pytest.mark.parametrize("max_iters", [0, 3])
def test_product_against_dense_f64_operators(product_lib, max_iters, solver, kw):
    """The HIP path against the same independent statement, without the oracle in between (FAST pair arithmetic: v_rsq / v_rcp
    approximations, the bars ten times the oracle's)."""
    scn, pos, mass, vel, P = _case(max_iters, solver, **kw)
    planes = sc.boundary_planes(scn.boundary, P.init_boundary_handler)
    g = ffi.Context(product_lib, len(mass), planes)
    _compare(g, pos, mass, vel, P, max_iters, 10.0, planes if kw.get("wall") else ())


# ------------------------------------------------------------------------------------------------------------------------------
# level estimation (before advection): detection by the empty 50-degree cone, Jacobi propagation, smoothing at the advected positions
#   lists of range k = level_estimation_range / 1.9 smoothing lengths               simulation.rs:2018-2046
#   n_i = -sum_j m_i / rho_0 grad W_ij; fewer than 3 list entries: surface (+ flag); |n|^2 < 1e-5: interior; closer than 1.5 h_i to a
#   wall (unless boundary_is_fluid_surface): interior; else interior iff some j has (x_j - x_i) / (|x_j - x_i| + 1e-6) . n / |n| > cos 50
#                                                                                      simulation.rs:540-612
#   sweeps: an interior particle with surface neighbours (state of the PREVIOUS sweep) takes max_j (level_j - |x_j - x_i|), until a
#   sweep assigns nothing; the stash after the detection / after the first sweep      simulation.rs:725-801, 886-893
#   smoothing: Shepard average of max(level, -maximum_surface_distance) (interior: the bound) with m_j / rho_j W(x'_ij, h_ij) over the
#   k = 2 lists of the step's start, at the advected positions x'                      simulation.rs:803-857, 2710-2721
# ------------------------------------------------------------------------------------------------------------------------------
def dense_level(pos, mass, P, planes=()):
    pos, mass = pos.astype(np.float64), mass.astype(np.float64)
    n = len(mass)
    h = 1.9 * np.sqrt(mass / P.rest_density / np.pi)
    d = pos[:, None, :] - pos[None, :, :]
    r = np.sqrt((d ** 2).sum(2))
    hij = 0.5 * (h[:, None] + h[None, :])
    ext = r < hij * (P.level_estimation_range / 1.9)
    q = r / (2.0 * hij)
    nf = 10.0 / (7.0 * np.pi * hij ** 2)
    dw = np.where(q < 0.5, 18.0 * q ** 2 - 12.0 * q, np.where(q < 1.0, -6.0 * (1.0 - q) ** 2, 0.0))
    with np.errstate(invalid="ignore", divide="ignore"):
        unit = np.where((q > 1.0e-5)[:, :, None], d / r[:, :, None], 0.0)
    G = (nf * dw / (2.0 * hij) * ext)[:, :, None] * unit
    normal = -(mass / P.rest_density)[:, None] * G.sum(1)
    wall_dist = np.full(n, np.inf)
    for (nx, ny, delta) in planes:
        wall_dist = np.minimum(wall_dist, nx * pos[:, 0] + ny * pos[:, 1] + delta)
    thr = np.cos(50.0 * np.pi / 180.0)
    surface, insufficient = np.zeros(n, bool), np.zeros(n, bool)
    for i in range(n):
        js = np.nonzero(ext[i])[0]
        if len(js) < 3:
            surface[i] = insufficient[i] = True
        elif (normal[i] ** 2).sum() < 0.00001:
            pass
        elif not P.boundary_is_fluid_surface and wall_dist[i] < h[i] * 1.5:
            pass
        else:
            nn = normal[i] / np.sqrt((normal[i] ** 2).sum())
            xji = -d[i, js] / (r[i, js] + 0.000001)[:, None]
            surface[i] = not ((xji @ nn) > thr).any()
    level = np.where(surface, 0.0, np.nan)
    first = level.copy()
    middle, sweeps = None, 0
    while True:
        have = ~np.isnan(level)
        est = np.where((ext & have[None, :]), level[None, :] - r, -np.inf).max(1)
        new = np.where(have, level, np.where(np.isfinite(est), est, np.nan))
        changed = (~have & ~np.isnan(new)).any()
        level = new
        sweeps += 1
        if sweeps == 1:
            middle = level.copy()
        if not changed:
            break
    return dict(surface=surface, insufficient=insufficient, first=first, middle=middle, level=level, sweeps=sweeps)


def dense_smooth(level, step, mass, P):
    x = step["position"]
    d = x[:, None, :] - x[None, :, :]
    r = np.sqrt((d ** 2).sum(2))
    hij, nb = step["_hij"], step["_nb"]
    q = r / (2.0 * hij)
    w = np.where(q < 0.5, 6.0 * (q ** 3 - q ** 2) + 1.0, np.where(q < 1.0, 2.0 * (1.0 - q) ** 3, 0.0))
    W = 10.0 / (7.0 * np.pi * hij ** 2) * w * nb
    msd = P.maximum_surface_distance
    dist = np.where(np.isnan(level), -msd, np.maximum(level, -msd))
    vol = (mass.astype(np.float64) / step["density"])[None, :] * W
    return (vol * dist[None, :]).sum(1) / vol.sum(1)


def _compare_level(ctx, stash_mode, tol, wall):
    scn, pos, mass, vel, P = _case(2, "HybridDFSPH", wall=wall, level_estimation_method="EmptyAngle", maximum_surface_distance=0.2)
    planes = sc.boundary_planes(scn.boundary, P.init_boundary_handler)
    compare_level_on(ctx, pos, mass, vel, P, planes, stash_mode, tol, wall)


def compare_level_on(ctx, pos, mass, vel, P, planes, stash_mode, tol, wall, block=True):
    """one step of `ctx` with the EmptyAngle level estimation on the given scene against dense_level / dense_smooth; `wall`: the scene
    touches the walls (`planes` enter the step's restatement too); `block`: the scene is one block the field reaches all of"""
    assert P.level_estimation_method == "EmptyAngle" and not P.level_estimation_after_advection and not P.boundary_is_fluid_surface
    P.fill_stash_with = stash_mode
    L = load_oracle().lib
    ctx.upload(mass, pos, vel)
    st = ctx.step(P.to_ffi())
    lv = dense_level(pos, mass, P, planes)
    step = dense_step(pos, mass, vel, P, float(st.dt), 3, planes if wall else (), lambda d: float(L.oracle_lambda2(d)), lambda d: float(L.oracle_dlambda2(d)))
    n = len(mass)
    assert 30 < lv["surface"].sum() < n // 2 and lv["sweeps"] >= 4
    if block:
        assert np.isnan(lv["level"]).sum() == 0                                        # the field reaches every particle of this block
    assert (lv["level"] < -P.maximum_surface_distance).sum() > 10                      # ... and some lie below the bound the smoothing clamps to
    assert np.array_equal(ctx.download("flag_is_fluid_surface").astype(bool), lv["surface"])
    assert np.array_equal(ctx.download("flag_insufficient_neighs").astype(bool), lv["insufficient"])
    ref_stash = lv["first"] if stash_mode == "SurfaceDistanceFirstIteration" else lv["middle"]
    ref_stash = np.where(np.isnan(ref_stash), -P.maximum_surface_distance, ref_stash)
    assert np.abs(ctx.download("stash") - ref_stash).max() <= 2e-6 * tol * max(np.abs(ref_stash).max(), 1e-30)
    sm = dense_smooth(lv["level"], step, mass, P)
    for f in ("level_estimation", "level_old"):
        assert np.abs(ctx.download(f) - sm).max() <= 5e-6 * tol * np.abs(sm).max(), f
    # classify_particles (adaptivity/mod.rs:24-59) from LevelEstimationState::target_mass (simulation.rs:213-237), three sizing functions
    for sizing in ("Mass", "Radius", "Radius2"):
        Pc = P.replace(sizing_function=sizing, particle_radius_fine=0.012, particle_radius_base=0.03)
        ctx.classify(Pc.to_ffi())
        t = np.maximum(sm, -Pc.maximum_surface_distance) / -Pc.maximum_surface_distance
        vol = lambda rad: np.pi * rad * rad                                            # noqa: E731
        if sizing == "Mass":
            target = (vol(0.012) * (1.0 - t) + vol(0.03) * t) * Pc.rest_density
        else:
            tt = t if sizing == "Radius" else np.sqrt(t)
            target = vol(0.012 * (1.0 - tt) + 0.03 * tt) * Pc.rest_density
        mrel = mass.astype(np.float64) / target
        cls = np.where(mrel <= 0.5, 0, np.where(mrel <= 1.0 / 1.1, 1, np.where(mrel < 1.1, 2, np.where(mrel < 2.0, 3, 4))))
        near = np.min(np.abs(mrel[:, None] - np.array([0.5, 1.0 / 1.1, 1.1, 2.0])[None, :]), 1) < 1e-4 * tol
        got = ctx.download("particle_size_class")
        assert len(np.unique(cls)) >= 4, sizing
        assert np.array_equal(got[~near], cls[~near]), sizing


@pytest.mark.parametrize("wall", [False, True])
@pytest.mark.parametrize("stash_mode", ["SurfaceDistanceFirstIteration", "SurfaceDistanceMiddle"])
def test_oracle_level_estimation_against_dense_restatement(stash_mode, wall):
    scn, pos, mass, vel, P = _case(2, "HybridDFSPH", wall=wall)
    o = ffi.Context(load_oracle(), len(mass), sc.boundary_planes(scn.boundary, P.init_boundary_handler))
    _compare_level(o, stash_mode, 1.0, wall)


@pytest.mark.gpu
@pytest.mark.parametrize("wall", [False, True])
@pytest.mark.parametrize("stash_mode", ["SurfaceDistanceFirstIteration", "SurfaceDistanceMiddle"])
def test_product_level_estimation_against_dense_restatement(product_lib, stash_mode, wall):
    scn, pos, mass, vel, P = _case(2, "HybridDFSPH", wall=wall)
    g = ffi.Context(product_lib, len(mass), sc.boundary_planes(scn.boundary, P.init_boundary_handler))
    _compare_level(g, stash_mode, 10.0, wall)


@pytest.mark.parametrize("which", ["oracle", pytest.param("product", marks=pytest.mark.gpu)])
def test_cfl_time_step_against_its_formula(which, request):
    """dt = min(max_dt, cfl_factor sqrt(min_i (2 h_i)^2 / (|v_i|^2 + 0.01)))   (simulation.rs:2182-2191), the CFL branch active"""
    scn, pos, mass, vel, P = _case(1, "IISPH")
    P = P.replace(max_dt=1.0)
    vel = (vel * 40.0).astype(np.float32)
    lib = load_oracle() if which == "oracle" else request.getfixturevalue("product_lib")
    ctx = ffi.Context(lib, len(mass), sc.boundary_planes(scn.boundary, P.init_boundary_handler))
    ctx.upload(mass, pos, vel)
    st = ctx.step(P.to_ffi())
    h = 1.9 * np.sqrt(mass.astype(np.float64) / P.rest_density / np.pi)
    dt = P.cfl_factor * np.sqrt(((2.0 * h) ** 2 / ((vel.astype(np.float64) ** 2).sum(1) + 0.01)).min())
    assert dt < 0.5 * P.max_dt
    assert st.dt == pytest.approx(dt, rel=2e-6)
