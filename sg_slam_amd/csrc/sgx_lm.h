// sgx_lm.h — the Levenberg-Marquardt control loop, once: statement-for-statement OptimizationAlgorithmLevenberg::solve (G/core/optimization_algorithm_levenberg.cpp:61-164,
// G = src/sg-slam/Thirdparty/g2o/g2o) around one optimizer.optimize(iterations) call.  Host only; used by the bundle adjustments and the essential-graph optimisation
// (sgx_ba.cpp), which differ in the hooks of their problem object and in nothing of the control:
//   bool stopped()                      the caller's stop flag (checked before an iteration and between the trials of one)
//   int  chi2(double *chi)              activeRobustChi2 of the current estimate
//   int  linearize()                    buildSystem
//   int  initial_lambda(double *l)      computeLambdaInit (after the first linearisation)
//   int  trial(double lambda, LmTrial*) push, damp, solve, update, computeScale, chi2 of the new estimate; ok = 0: the factorisation failed
//   int  reject()                       pop: back to the estimate before the trial
// Every hook but stopped() returns an sgx_status; anything but SGX_OK ends the optimisation with that status.
#pragma once
#include <float.h>
#include <cmath>

struct LmTrial { int ok = 1; double scale = 0, chi = 0; };
struct LmResult { int iterations = 0; double chi_first = 0, chi_last = 0; };      // iterations done; chi2 before the first and after the last of them

template <class Problem> static int sgx_lm_solve(Problem &p, int iterations, LmResult *out)
{
    double lambda = -1, ni = 2; int nBadLM = 0, rc;
    for (int it = 0; it < iterations; it++) {
        if (p.stopped()) break;
        double currentChi = 0; if ((rc = p.chi2(&currentChi)) != SGX_OK) return rc;
        if (it == 0) out->chi_first = currentChi;
        double tempChi = currentChi; const double iniChi = currentChi;
        if ((rc = p.linearize()) != SGX_OK) return rc;
        if (it == 0) { if ((rc = p.initial_lambda(&lambda)) != SGX_OK) return rc; ni = 2; nBadLM = 0; }
        double rho = 0; int qmax = 0;
        do {
            LmTrial t; if ((rc = p.trial(lambda, &t)) != SGX_OK) return rc;
            double scale = t.scale; tempChi = t.chi;
            if (!t.ok) tempChi = DBL_MAX;
            rho = currentChi - tempChi;
            scale += 1e-3; rho /= scale;
            if (rho > 0 && std::isfinite(tempChi)) {
                const double r21 = 2 * rho - 1;
                double alpha = 1. - r21 * r21 * r21; alpha = alpha < 2. / 3. ? alpha : 2. / 3.;
                lambda *= (alpha > 1. / 3. ? alpha : 1. / 3.); ni = 2; currentChi = tempChi;
            } else {
                lambda *= ni; ni *= 2;
                if ((rc = p.reject()) != SGX_OK) return rc;
            }
            qmax++;
        } while (rho < 0 && qmax < 10 && !p.stopped());
        out->iterations = it + 1; out->chi_last = currentChi;
        if (qmax == 10 || rho == 0) break;
        if ((iniChi - currentChi) * 1e3 < iniChi) nBadLM++; else nBadLM = 0;
        if (nBadLM >= 3) break;
    }
    return SGX_OK;
}
