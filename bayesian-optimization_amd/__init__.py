"""bogp -- MI355X-native GP-surrogate + batch-acquisition engine behind the `bayes_optim` protocols.

The directory is named `bayesian-optimization_amd/`; import it as `bogp` (bogp/__init__.py is the alias).

  bogp.GaussianProcess           <-> bayes_optim.surrogate.GaussianProcess      (fit / predict / gradient)
  bogp.acquisition.{EI,PI,EpsilonPI,UCB,MGFI} <-> bayes_optim.acquisition.acquisition_fun.*
  bogp.EHVI                      <-> bayes_optim.multi_objective.analytic.EHVI (MOBO's criterion; one device pass)
                                 (on a multi-target GaussianProcess, or on a RandomForest fitted on y (N, m))
  bogp.Constrained               EI / PI / EpsilonPI / MGFI weighted by the probability that modelled constraints hold: the
                                 h_vals / g_vals the reference's tell() accepts and drops (one device pass, bogp_sweep_constrained)
  bogp.ConstrainedEHVI           EHVI of the feasible front weighted by the same probability: the h_vals / g_vals BaseMOBO.tell leaves
                                 as a TODO (mobo.py:117-118; one device pass, bogp_sweep_ehvi_constrained);
                                 bogp.constrained_ehvi_believer_batch: its q-point proposals by the Kriging believer
  bogp.pareto                    Pareto front + cell decomposition of the non-dominated region (numpy)
  bogp.RandomForest              <-> bayes_optim.surrogate.RandomForest        (scikit-learn fits, the device predicts;
                                 bogp.forest: packing, mixed-space sweep; built on first access, sklearn imported lazily)
  bogp.optim.argmax_restart      <-> bayes_optim.acquisition.optim.argmax_restart (+ optimizer="sweep")
  bogp.trend                     <-> bayes_optim.surrogate.trend
  bogp.thompson                  posterior sample paths (GaussianProcess.sampling_posterior, stubs in the reference) and
                                 bogp.thompson_batch: q-point proposals by Thompson sampling;
                                 bogp.constrained_thompson_batch: the same under modelled constraints (joint paths)
  bogp.install(bayes_optim)      re-points the reference's three extension points, ParallelBO's q-criterion loop and
                                 MOBO's acquisition (EHVI under the sweep family)
  bogp._lib.Engine               ctypes binding of libbogp.so (include/bogp.h)

Every numerical step runs on the GPU through libbogp.so; importing works anywhere, but creating an engine without
a gfx950 device (or without the built library) raises -- there is no CPU fallback.
"""
__version__ = "0.1.0"

from . import _lib, acquisition, distributed, forest, integration, lift, optim, pareto, thompson  # noqa: E402,F401
from . import prior_mean as trend  # noqa: E402,F401
from .acquisition import EHVI, EI, MGFI, PI, UCB, Constrained, ConstrainedEHVI, EpsilonPI  # noqa: E402,F401
from .optim import argmax_restart, batch_argmax, believer_batch, constrained_believer_batch, constrained_ehvi_believer_batch, constrained_thompson_batch, device_sample, ehvi_believer_batch, sweep_argmax, sweep_generated, sweep_topk, sweep_topk_generated, thompson_batch  # noqa: E402,F401
from .integration import feasible_front, feasible_xopt, install, uninstall  # noqa: E402,F401
from .lift import Lift  # noqa: E402,F401
from .surrogate import GaussianProcess  # noqa: E402,F401


def __getattr__(name):  # bogp.RandomForest subclasses scikit-learn's regressor: built (and scikit-learn imported) on first access
    if name == "RandomForest":
        return forest.RandomForest
    raise AttributeError("module %r has no attribute %r" % (__name__, name))
