"""What the MD drivers of this directory share (nve_water.py, nvt_water.py, npt_water.py, mts_water.py): the water force field's bonded
constants, the command-line arguments, the calculators with their Verlet lists, the `forces` closure and the `box_gradient`
closure of the NPT driver, the minimisation that relaxes the synthetic box before a run (capped steepest descent, or
--minimizer fire: admp_amd.md.FireMinimizer; minimize_water.py runs the two side by side), and the start of the rigid-water
drivers (rigid_water.py, npt_water.py --rigid)."""
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from admp_amd import settings, systems as S                                                   # noqa: E402

KB = 0.0083144626          # kJ/mol/K
MASS = (15.999, 1.008, 1.008)
K_BOND, R0 = 376560.0 / 100.0, 0.9572          # kJ/mol/A^2 (xml: per nm^2)
K_ANG, TH0 = 460.24, 1.82421813418


def bonded(pos, n_mol):
    """torch restatement of the bonded terms (the checker of tests/test_gpu_examples.py; the loop uses admp_amd.md)"""
    m = pos.reshape(n_mol, 3, 3)
    a, b = m[:, 1] - m[:, 0], m[:, 2] - m[:, 0]
    ra, rb = a.norm(dim=1), b.norm(dim=1)
    th = torch.acos(torch.clamp((a * b).sum(1) / (ra * rb), -1.0, 1.0))
    return 0.5 * K_BOND * ((ra - R0) ** 2 + (rb - R0) ** 2).sum() + 0.5 * K_ANG * ((th - TH0) ** 2).sum()


def add_arguments(ap):
    ap.add_argument('--waters', type=int, default=1024)
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--dt', type=float, default=0.5, help='fs')
    ap.add_argument('--pol', action='store_true')
    ap.add_argument('--single', action='store_true')
    ap.add_argument('--rebuild', type=int, default=10)
    ap.add_argument('--prune', type=int, default=0, help='steps between prunings of an inner list (admp_prune_pairs; 0: walk the whole skin '
                    'list).  Pays from ~200k atoms on; the drift of an NVE run grows with it: the multipolar kernels evaluate every listed '
                    'pair, and the set of pairs beyond rc changes at every prune')
    ap.add_argument('--cut', action='store_true', help='set_cutoff(rc) on the three calculators: every term is then the one of the '
                    'exact-rc list whatever the age of the skin list (default off: every listed pair counts, as in the reference)')
    ap.add_argument('--minimize', type=int, default=200)
    ap.add_argument('--minimizer', choices=('sd', 'fire'), default='sd', help='sd: capped steepest descent (0.02 A per evaluation, one host '
                    'read each); fire: admp_amd.md.FireMinimizer (one C call per iteration, the control loop on the device); the '
                    'rigid-water drivers then minimise a second time ON the constraints')
    ap.add_argument('--temp', type=float, default=300.0)
    ap.add_argument('--mesh', type=int, default=0, help='PME mesh size per dimension (0: the reference rule)')
    ap.add_argument('--log', type=int, default=10, help='steps between energy records (each costs two host reads)')
    ap.add_argument('--thresh', type=float, default=1e-2, help='SCF threshold of --pol (the reference default 10 does not conserve energy)')
    ap.add_argument('--dipoles', type=int, default=0, metavar='N', help='record the molecular and cell dipoles every N steps (0: off; '
                    'admp_amd.md.DipoleRecorder: two small kernels per record, nothing read back until the run ends) and print the mean '
                    'molecular dipole, its permanent and induced shares and the dielectric constant of the run')
    ap.add_argument('--rdf', type=int, default=0, metavar='N', help='add a frame to the radial distribution functions every N steps (0: '
                    'off; admp_amd.md.RdfRecorder: one C call per frame, integer counters on the device, nothing read back until the run '
                    'ends) to r_max = min(10 A, 0.49 x the smallest cell height) in bins of 0.05 A, and print the first g_OO peak, the '
                    'minimum after it, the O-O coordination number up to there and the first intermolecular g_OH peak')
    ap.add_argument('--rdf-out', default='', metavar='FILE', help='write r, g_OO, g_OH, g_HH of --rdf as text')
    ap.add_argument('--msd', type=int, default=0, metavar='N', help='record a frame of the mean-square displacements and velocity '
                    'autocorrelations of O and H every N steps (0: off; admp_amd.md.CorrelationRecorder: a ring of the last --msd-lags '
                    'frames on the device, one C call per frame, nothing read back until the run ends) and print the self-diffusion '
                    'coefficient of oxygen (Einstein fit over the second half of the lags, and Green-Kubo), the large jumps counted and, '
                    'when the lag window resolves it, the O-H stretch peak of the hydrogen density of states')
    ap.add_argument('--msd-lags', type=int, default=512, metavar='L', help='lags of --msd: the correlation window is L x N x dt')
    ap.add_argument('--msd-out', default='', metavar='FILE', help='write t, msd_O, msd_H, vacf_O, vacf_H of --msd as text')
    start = ap.add_mutually_exclusive_group()
    start.add_argument('--aspc', type=int, default=-1, choices=(0, 1, 2, 3, 4), metavar='K', help='always-stable predictor-corrector dipoles '
                       'of order K in the library (ADMPPmeForce.set_aspc, switched on after the minimiser): after K + 2 warm-up steps '
                       'every step is the predictor and --aspc-corr damped Jacobi steps, 1 + --aspc-corr field evaluations, no SCF to '
                       '--thresh and no residual read')
    ap.add_argument('--aspc-corr', type=int, default=1, metavar='N', help='corrector steps of --aspc (1: Kolafa\'s scheme)')
    start.add_argument('--predict', type=int, default=0, choices=(0, 1, 2, 3), help='start the SCF from a polynomial predictor over the last k + 1 '
                    'converged dipoles (Kolafa\'s always-stable predictor coefficients: k = 1 is 2 U(n-1) - U(n-2)) instead of U(n-1): a few '
                    'tensor operations per step; at a tight threshold it saves one to two field evaluations per step')


def add_thermostat_arguments(ap):
    ap.add_argument('--thermostat', choices=('langevin', 'vrescale'), default='langevin', help='langevin: the friction and noise of '
                    'the integrator (--friction); vrescale: stochastic velocity rescaling (admp_amd.md.VRescale) on the integrator at '
                    'friction 0 -- one factor for all velocities per step, so diffusion and dipole dynamics are not damped')
    ap.add_argument('--tau-t', type=float, default=100.0, help='fs: relaxation time of --thermostat vrescale')


def drift_of(log, conserved=lambda r: r[1] + r[2] - r[-1]):
    """'d kJ/mol over n steps' of the conserved quantity (E_pot + E_kin - heat of records (step, E_pot, E_kin, ..., heat)) between
    the first and the last record"""
    return '%+.4f kJ/mol over %d steps' % (conserved(log[-1]) - conserved(log[0]), log[-1][0] - log[0][0])


def setup(opt):
    """calculators, lists and forces of the box of opt.waters molecules; returns a namespace with pos (device tensor), box,
    n_mol, dtype, pme (the calculator that lends its handle and stream to the integrator), nbl, forces, epot_now, state; for
    the NPT driver also tt (the pair-interaction object), par (the parameter tensors) and box_gradient.  `box` is ONE ndarray
    that every closure reads at each call: a barostat that scales it in place changes the cell for all of them."""
    settings.PRECISION = 'single' if opt.single else 'double'
    if opt.pol:
        settings.POL_CONV = opt.thresh      # a tight SCF: the reference's default (10) is too loose for energy conservation
        settings.MAX_N_POL = 60
    from admp_amd.pme import ADMPPmeForce
    from admp_amd.disp_pme import ADMPDispPmeForce
    from admp_amd.pairwise import generate_pairwise_interaction, TT_damping_qq_c6_kernel, value_and_grad
    from admp_amd.md import HarmonicBonded

    n_mol = opt.waters
    pos0, box = S.synthetic_water_box(n_mol, seed=20240)
    at, ai, cov = S.water_topology(n_mol)
    par = S.water_parameters(n_mol, polarizable=opt.pol)
    dt = torch.float32 if opt.single else torch.float64
    dev = 'cuda'
    rc, skin = 4.0, 1.0
    pme = ADMPPmeForce(box, at, ai, cov, rc, 1e-4, 2, lpol=opt.pol)
    disp = ADMPDispPmeForce(box, cov, rc, 1e-4, 10)
    if opt.mesh:
        for obj in (pme, disp):
            for k in ('K1', 'K2', 'K3'):
                obj.update_env(k, opt.mesh)
    tt_obj = generate_pairwise_interaction(TT_damping_qq_c6_kernel, cov, static_args={})
    tt = value_and_grad(tt_obj)
    if opt.cut:
        for obj in (pme, disp, tt_obj):
            obj.set_cutoff(rc)
    o = 3 * np.arange(n_mol)
    bonds = np.stack([np.concatenate([o, o]), np.concatenate([o + 1, o + 2])], axis=1)
    angles = np.stack([o + 1, o, o + 2], axis=1)
    bond = HarmonicBonded(3 * n_mol, bonds, np.tile([K_BOND, R0], (2 * n_mol, 1)), angles, np.tile([K_ANG, TH0], (n_mol, 1)))

    class Lists:
        """Verlet lists with a skin, rebuilt every --rebuild steps (the pair kernels have no cutoff test of their own,
        like the reference).  The PME calculator compiles the neighbour table on the GPU straight from the positions
        (`update_neighbors`, search fused with the table build); the other two borrow it (`share_neighbors` -- the
        reference's drivers hand one `pairs` array to every force object) and all are then called with pairs=None."""
        def allocate(self, p):
            pme.update_neighbors(p, box, rc=rc + skin)
            for obj in (disp, tt_obj):
                obj.share_neighbors(pme)
            return None

        def prune(self, p):
            """inner list (admp_prune_pairs): the entries of the skin list within rc + the share of the skin the atoms can use up
            until the next prune; the multipolar kernels evaluate every listed pair, so a shorter list is less work"""
            pme.prune_neighbors(p, box, rc + skin * opt.prune / float(opt.rebuild))
    nbl = Lists()
    pos = torch.as_tensor(pos0, dtype=dt, device=dev)
    mass = torch.as_tensor(np.tile(MASS, n_mol), dtype=dt, device=dev)[:, None]
    T = lambda k: torch.as_tensor(par[k], dtype=dt, device=dev)      # noqa: E731
    Q, pol, thole, cl = T('Q_local'), T('pol'), T('tholes'), T('c_list')
    a_, b_, q_, c6 = T('a_list'), T('b_list'), T('q_list'), cl[:, 0].contiguous()
    mS, pS, dS = par['mScales'], par['pScales'], par['dScales']
    state = {'U': None}

    def forces(p, pairs, bonded=True):
        """(potential energy of the three calculators -- numbers they return anyway --, +dE/dr of everything); the bonded
        energy of this evaluation is in bond.energy_words (read by epot_now() when a line is logged).  bonded=False: the
        calculators alone, bond.energy_words untouched (mts_water.py: the integrator's kernel evaluates the bonded terms)"""
        if opt.pol:
            U0 = state['U']
            hist = state.setdefault('hist', [])
            if opt.predict and len(hist) == opt.predict + 1:
                coef = {1: (2.0, -1.0), 2: (2.5, -2.0, 0.5), 3: (2.8, -2.8, 1.2, -0.2)}[opt.predict]
                U0 = coef[0] * hist[-1]
                for c, Uh in zip(coef[1:], reversed(hist[:-1])):
                    U0 = U0 + c * Uh
            e1, g = pme.get_forces(p, box, pairs, Q, pol, thole, mS, pS, dS, U_init=U0)
            state['U'] = pme.U_ind
            if opt.predict:
                hist.append(state['U'])
                del hist[:-(opt.predict + 1)]
            state['cyc'] = state.get('cyc', 0) + pme.n_cycle + 1
            state['n'] = state.get('n', 0) + 1
            if state.get('aspc_on'):      # the steps after the warm-up are counted on their own
                state['aspc_calls'] += 1
                if state['aspc_calls'] > opt.aspc + 2:
                    state['aspc_cyc'] += pme.n_cycle + 1
                    state['aspc_n'] += 1
        else:
            e1, g = pme.get_forces(p, box, pairs, Q, mS)
        e2, g2 = disp.get_forces(p, box, pairs, cl, mS)
        e3, g3 = tt(p, box, pairs, mS, a_, b_, q_, c6)
        g.add_(g2).add_(g3)
        if bonded:
            bond.reset_energy()
            bond.add_forces(p, box, g)
        return e1 + e2 + e3, g

    def epot_now(e123):
        return float(e123) + bond.energy()

    def box_gradient(p, pairs, bonded=True):
        """dE/dbox (3,3) at fixed Cartesian positions summed over the four calculators, at the list and (--pol) from the
        dipoles of the last forces() call; four evaluations, used every --nbaro steps by npt_water.py.  bonded=False: the
        three calculators alone (npt_water.py --rigid has no bonded terms, or an angle term of its own)"""
        if opt.pol:
            d = pme.get_energy_and_box_gradient(p, box, pairs, Q, pol, thole, mS, pS, dS, U_init=state['U'])[1]
        else:
            d = pme.get_energy_and_box_gradient(p, box, pairs, Q, mS)[1]
        d = d + disp.get_energy_and_box_gradient(p, box, pairs, cl, mS)[1]
        d = d + tt_obj.get_energy_and_box_gradient(p, box, pairs, mS, a_, b_, q_, c6)[1]
        return d + bond.get_energy_and_box_gradient(p, box)[1] if bonded else d

    def start_aspc():
        """--aspc: switched on once the minimiser is done (every polarizable call is a time step from here on)"""
        if not opt.pol or opt.aspc < 0:
            return
        pme.set_aspc(opt.aspc, opt.aspc_corr)
        state.update(aspc_on=True, aspc_calls=0, aspc_cyc=0, aspc_n=0, cyc=0, n=0)

    def aspc_jump():
        """after anything that moves atoms discontinuously: the stored dipoles say nothing about the next step"""
        if state.get('aspc_on'):
            pme.reset_aspc()
            state['aspc_calls'] = 0

    def scf_lines():
        """the lines a --pol run prints about its SCF"""
        out = ['# mean SCF cycles per evaluation (thresh %g): %.1f' % (settings.POL_CONV, state['cyc'] / max(state['n'], 1))]
        if state.get('aspc_on'):
            i = pme.aspc_info()
            out.append('# ASPC order %d, %d corrector step(s), omega %.4f: %.2f field evaluations per step after the warm-up '
                       '(%d fixed-form, %d warm-up, %d fallback calls; residual at the last predicted dipoles %.3e)'
                       % (i['order'], i['n_corrector'], i['omega'], state['aspc_cyc'] / max(state['aspc_n'], 1), i['fixed'],
                          i['warmup'], i['fallback'], i['residual']))
        return out

    dip = {}

    def record_dipoles(step, p):
        """--dipoles N: every N steps one row with the dipoles of the last forces() call and one without them (the permanent
        share), each two small kernels on the calculator's stream; no host read"""
        n_rec = getattr(opt, 'dipoles', 0)
        if not n_rec or step % n_rec:
            return
        if not dip:
            from admp_amd.md import DipoleRecorder
            rows = (opt.steps + n_rec - 1) // n_rec
            labels, masses = np.repeat(np.arange(n_mol), 3), np.tile(MASS, n_mol)
            dip.update(full=DipoleRecorder(pme, labels, masses, rows), static=DipoleRecorder(pme, labels, masses, rows),
                       zero=torch.zeros_like(p), volumes=[])
        dip['full'].record(p, box, Q, state['U'] if opt.pol else None)
        dip['static'].record(p, box, Q, dip['zero'])
        dip['volumes'].append(abs(float(np.linalg.det(np.asarray(box, dtype=np.float64).reshape(3, 3)))))

    def dipole_lines():
        """the lines a --dipoles run prints when it ends (the one host read of each recorder)"""
        if not dip:
            return []
        from admp_amd.md import DEBYE_PER_E_ANGSTROM as D, dielectric_constant
        full, static = dip['full'].rows(), dip['static'].rows()
        mean, perm = D * (full[:, 9] / full[:, 12]).mean(), D * (static[:, 9] / static[:, 12]).mean()
        M = full[:, 0:3] + full[:, 3:6] + full[:, 6:9]
        eps = dielectric_constant(M, float(np.mean(dip['volumes'])), opt.temp)
        return ['# dipoles over %d records: mean molecular dipole %.4f D (permanent share %.4f D, induced share %.4f D); dielectric '
                'constant %.2f at %.1f K -- a few hundred steps do not converge the dielectric constant: the cell dipole relaxes over '
                'tens of picoseconds' % (len(full), mean, perm, mean - perm, eps, opt.temp)]

    rdf = {}

    def record_rdf(step, p):
        """--rdf N: every N steps the frame's O-O, O-H and H-H pair distances (pairs inside a molecule excluded) into the device
        histogram: one C call on the calculator's stream; no host read.  r_max is fixed at the first frame; a cell that shrinks
        below 2 r_max afterwards (NPT) is refused by the library"""
        n_rec = getattr(opt, 'rdf', 0)
        if not n_rec or step % n_rec:
            return
        if not rdf:
            from admp_amd.md import RdfRecorder
            h = np.asarray(box, dtype=np.float64).reshape(3, 3)
            inv = np.linalg.inv(h)
            r_max = min(10.0, 0.49 * float((1.0 / np.sqrt((inv * inv).sum(axis=0))).min()))
            rdf['rec'] = RdfRecorder(pme, np.tile([0, 1, 1], n_mol), r_max, max(int(round(r_max / 0.05)), 1), groups=np.repeat(np.arange(n_mol), 3))
        rdf['rec'].record(p, box)

    def rdf_lines():
        """the lines a --rdf run prints when it ends (the one host read of the recorder); writes --rdf-out"""
        if not rdf:
            return []
        rec = rdf['rec']
        r, g, n = rec.rdf()
        goo, goh, ghh = g[(0, 0)], g[(0, 1)], g[(1, 1)]
        if getattr(opt, 'rdf_out', ''):
            np.savetxt(opt.rdf_out, np.stack([r, goo, goh, ghh], axis=1), header='r/A g_OO g_OH g_HH (%d frames)' % rec.frames)
        info = rec.info()
        out = ['# rdf over %d frames: r_max %.3f A, %d bins of %.4f A, %s form, %d workgroups' % (rec.frames, rec.r_max, rec.n_bins,
                                                                                               rec.r_max / rec.n_bins, info['form'], info['workgroups'])]
        # the first maximum: the highest bin below 3.6 A (the first O-O shell of water ends near 3.3 A); the minimum after it: the
        # lowest bin between the peak and 1.6 x its position.  Bins of 0.05 A over a few frames are noisy: smoothed over 5 bins.
        sm = np.convolve(goo, np.ones(5) / 5.0, mode='same')
        first = r < 3.6
        if first.any() and sm[first].max() > 0:
            kp = int(np.argmax(np.where(first, sm, -1.0)))
            after = (r > r[kp]) & (r <= 1.6 * r[kp])
            km = int(np.argmin(np.where(after, sm, np.inf))) if after.any() else kp
            out.append('# g_OO: first maximum %.3f at %.3f A, first minimum %.3f at %.3f A, O-O coordination number up to the minimum '
                       '%.2f; g_OO is zero below %.3f A' % (sm[kp], r[kp], sm[km], r[km], n[(0, 0)][km],
                                                          r[np.nonzero(goo)[0][0]] - 0.5 * rec.r_max / rec.n_bins))
        smh = np.convolve(goh, np.ones(5) / 5.0, mode='same')
        inter = (r > 1.3) & (r < 2.5)      # the hydrogen-bond peak: beyond the (excluded) bond length, before the second shell
        if inter.any() and smh[inter].max() > 0:
            kh = int(np.argmax(np.where(inter, smh, -1.0)))
            out.append('# g_OH: first intermolecular maximum %.3f at %.3f A' % (smh[kh], r[kh]))
        return out

    tcf = {}

    def record_msd(step, p, v):
        """--msd N: every N steps positions and velocities into the device ring and the frame's correlations with every frame
        of the ring into the sums: one C call on the calculator's stream; no host read.  The velocities are those the driver holds
        where it records (after the force evaluation: v of the half step in the Verlet drivers)"""
        n_rec = getattr(opt, 'msd', 0)
        if not n_rec or step % n_rec:
            return
        if not tcf:
            from admp_amd.md import CorrelationRecorder
            tcf['rec'] = CorrelationRecorder(pme, np.tile([0, 1, 1], n_mol), opt.msd_lags, n_rec * opt.dt)
        tcf['rec'].record(p, v, box)

    def msd_lines():
        """the lines a --msd run prints when it ends (the host reads of the recorder); writes --msd-out"""
        if not tcf:
            return []
        from admp_amd.md import DIFFUSION_1E5_CM2_S, diffusion_einstein, diffusion_green_kubo, tcf_normalise, vdos
        rec = tcf['rec']
        t, msd, vacf = tcf_normalise(rec.sums(), rec.type_counts, rec.dt_fs)
        if getattr(opt, 'msd_out', ''):
            np.savetxt(opt.msd_out, np.stack([t, msd[0], msd[1], vacf[0], vacf[1]], axis=1),
                       header='t/fs msd_O/A^2 msd_H/A^2 vacf_O/(A/fs)^2 vacf_H/(A/fs)^2 (%d frames)' % rec.frames)
        info = rec.info()
        out = ['# msd over %d frames every %.2f fs: %d lags, %d workgroups, large_jumps %d'
               % (rec.frames, rec.dt_fs, rec.n_lags, info['workgroups'], info['large_jumps'])]
        have = int(min(rec.frames, rec.n_lags))      # lags with at least one origin
        if have >= 3:
            lo, hi = t[have // 2], t[have - 1]
            d_e = diffusion_einstein(t[:have], msd[0][:have], lo, hi) * DIFFUSION_1E5_CM2_S
            d_gk = diffusion_green_kubo(t[:have], vacf[0][:have])[0] * DIFFUSION_1E5_CM2_S
            out.append('# D_O: Einstein %.4f (fit over %.1f..%.1f fs), Green-Kubo %.4f, in 1e-5 cm^2/s' % (d_e, lo, hi, d_gk))
            # the O-H stretch: resolved when the bins are finer than 250 1/cm and reach beyond 2500 1/cm
            if vacf[1][0] > 0:
                w, S = vdos(t[:have], vacf[1][:have])
                if w[1] - w[0] <= 250.0 and w[-1] > 2500.0:
                    k = int(np.argmax(np.where(w > 2500.0, S, -np.inf)))
                    out.append('# vdos_H: highest peak above 2500 cm^-1 at %.0f cm^-1 (bins of %.0f cm^-1)' % (w[k], w[1] - w[0]))
        return out

    par_t = types.SimpleNamespace(Q=Q, pol=pol, thole=thole, c_list=cl, a=a_, b=b_, q=q_, c6=c6, mS=mS, pS=pS, dS=dS)
    return types.SimpleNamespace(n_mol=n_mol, box=box, pos=pos, dtype=dt, mass=mass, pme=pme, disp=disp, bond=bond, nbl=nbl,
                                 forces=forces, epot_now=epot_now, state=state, tt=tt_obj, par=par_t, box_gradient=box_gradient,
                                 start_aspc=start_aspc, aspc_jump=aspc_jump, scf_lines=scf_lines, record_dipoles=record_dipoles,
                                 dipole_lines=dipole_lines, record_rdf=record_rdf, rdf_lines=rdf_lines, record_msd=record_msd,
                                 msd_lines=msd_lines)


def minimize_fire(w, opt, pos, gradient=None, epot=None, constraints=None, label='minimize'):
    """opt.minimize iterations of admp_amd.md.FireMinimizer on a copy of pos, the list rebuilt every opt.rebuild iterations;
    gradient (default: w.forces, everything) -> (e, grad) and epot (default: w.epot_now) -> the energy of e for a printed line;
    constraints: a Constraints to minimise on.  Returns (pos, pairs, e, grad) at the end, like minimize()."""
    from admp_amd.md import FireMinimizer
    nbl = w.nbl
    gradient, epot = gradient or w.forces, epot or w.epot_now
    pos = pos.clone().contiguous()
    fm = FireMinimizer(w.pme, 3 * w.n_mol, np.tile(MASS, w.n_mol), constraints=constraints)
    pairs = nbl.allocate(pos)
    for it in range(opt.minimize):
        e, grad = gradient(pos, pairs)
        if it % 50 == 0 or it == opt.minimize - 1:
            print('%s %4d  Epot %14.4f' % (label, it, epot(e)))
        fm.step(pos, grad, 0.0, w.box if constraints is not None else None)
        if (it + 1) % opt.rebuild == 0:
            pairs = nbl.allocate(pos)
    info = fm.info()
    if info['failed']:
        raise FloatingPointError('FIRE: a force or a velocity is not finite')
    print('# FIRE: %d iterations, %d uphill, dt %.3f fs, largest |F_i| before the last step %.3f kJ/mol/A'
          % (info['iterations'], info['uphill_steps'], info['dt'], info['fmax']))
    pairs = nbl.allocate(pos)
    e, grad = gradient(pos, pairs)
    return pos, pairs, e, grad


def minimize(w, opt, pos):
    """the synthetic box is not equilibrated: it is relaxed first, by capped steepest descent or (--minimizer fire) by FIRE;
    returns (pos, pairs, e123, grad) at the end"""
    if getattr(opt, 'minimizer', 'sd') == 'fire':
        return minimize_fire(w, opt, pos)
    nbl, forces, epot_now = w.nbl, w.forces, w.epot_now
    pairs = nbl.allocate(pos)
    e123, grad = forces(pos, pairs)
    for it in range(opt.minimize):
        pos = pos - grad * (0.02 / max(float(grad.norm(dim=1).max()), 1e-12))
        if (it + 1) % opt.rebuild == 0:
            pairs = nbl.allocate(pos)
        e123, grad = forces(pos, pairs)
        if it % 50 == 0 or it == opt.minimize - 1:
            print('minimize %4d  Epot %14.4f' % (it, epot_now(e123)))
    pairs = nbl.allocate(pos)
    e123, grad = forces(pos, pairs)
    return pos.contiguous(), pairs, e123, grad


def rigid_start(w, opt, masses):
    """what rigid_water.py and npt_water.py --rigid share: the constraints of rigid water (O-H, O-H and H-H; opt.bonds_only: the
    O-H bonds, with the harmonic angle as a HarmonicBonded of its own), the constrained integrator, the gradient closure
    without the bonded terms, and the start -- the flexible minimisation, the positions projected onto the constraints,
    Maxwell-Boltzmann velocities projected likewise and rescaled to opt.temp over the constrained degrees of freedom.  Returns
    a namespace: con, angle, integ, tol, n_dof, gradient, epot_now, constraint_error, pos, vel, pairs, e123, grad."""
    from admp_amd.md import Constraints, ConstrainedLangevin, HarmonicBonded, maxwell_boltzmann
    n_mol, box, nbl = w.n_mol, w.box, w.nbl
    tol = opt.tol or (1e-6 if opt.single else 1e-8)
    o = 3 * np.arange(n_mol)
    pairs = [np.stack([o, o + 1], axis=1), np.stack([o, o + 2], axis=1)]
    lengths = [np.full(n_mol, R0), np.full(n_mol, R0)]
    if not opt.bonds_only:
        pairs.append(np.stack([o + 1, o + 2], axis=1))
        lengths.append(np.full(n_mol, 2.0 * R0 * np.sin(0.5 * TH0)))
    pairs = np.stack(pairs, axis=1).reshape(-1, 2)          # a molecule's constraints side by side
    lengths = np.stack(lengths, axis=1).reshape(-1)
    con = Constraints(3 * n_mol, pairs, lengths, masses, tolerance=tol)
    angle = None
    if opt.bonds_only:
        angle = HarmonicBonded(3 * n_mol, np.zeros((0, 2)), np.zeros((0, 2)), np.stack([o + 1, o, o + 2], axis=1),
                               np.tile([K_ANG, TH0], (n_mol, 1)))
    integ = ConstrainedLangevin(con, opt.dt, opt.temp, opt.friction, opt.seed)
    pi, pj = (torch.as_tensor(pairs[:, k], device='cuda') for k in (0, 1))
    d_t = torch.as_tensor(lengths, dtype=torch.float64, device='cuda')

    def gradient(p, prs):
        """the calculators without the bonded terms, plus the harmonic angle of --bonds-only"""
        e, g = w.forces(p, prs, bonded=False)
        if angle is not None:
            angle.reset_energy()
            angle.add_forces(p, box, g)
        return e, g

    def epot_now(e):
        return float(e) + (angle.energy() if angle is not None else 0.0)

    def constraint_error(p):
        """largest | |x_j - x_i| - d | / d, minimum image, in double on the device"""
        h = torch.as_tensor(np.asarray(box, dtype=np.float64).reshape(3, 3), device='cuda')
        s = (p[pj].double() - p[pi].double()) @ torch.linalg.inv(h)
        d = ((s - torch.round(s)) @ h).norm(dim=1)
        return float(((d - d_t).abs() / d_t).max())

    pos, _, _, _ = minimize(w, opt, w.pos)                                 # flexible, as the other drivers
    print('# constraint error before the projection %.3e' % constraint_error(pos))
    con.project_positions(pos, box)
    if getattr(opt, 'minimizer', 'sd') == 'fire':      # a second stage ON the constraints, without the bonded terms they replace
        pos, _, _, _ = minimize_fire(w, opt, pos, gradient=gradient, epot=epot_now, constraints=con, label='minimize (rigid)')
        print('# constraint error after the constrained minimisation %.3e' % constraint_error(pos))
    pairs_l = nbl.allocate(pos)
    e123, grad = gradient(pos, pairs_l)
    vel = maxwell_boltzmann(con, masses, opt.temp, opt.seed)
    con.project_velocities(pos, vel, box, opt.dt)
    n_dof = 9 * n_mol - con.n_constraints
    m_t = torch.as_tensor(masses, dtype=w.dtype, device='cuda')[:, None]
    t_now = float((m_t * vel * vel).sum()) / ConstrainedLangevin.ACC / (n_dof * KB)
    if t_now > 0:
        vel *= float(np.sqrt(opt.temp / t_now))
    print('# %d constraints (%s), tolerance %.1e; start: constraint error %.3e, T %.1f K over %d degrees of freedom, failures %d'
          % (con.n_constraints, 'O-H bonds, harmonic angle' if opt.bonds_only else 'rigid water', tol, constraint_error(pos),
             opt.temp if t_now > 0 else 0.0, n_dof, con.failures()))
    con.reset_failures()
    return types.SimpleNamespace(con=con, angle=angle, integ=integ, tol=tol, n_dof=n_dof, gradient=gradient, epot_now=epot_now,
                                 constraint_error=constraint_error, pos=pos, vel=vel, pairs=pairs_l, e123=e123, grad=grad)
