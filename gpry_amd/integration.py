"""Rebind GPry's class names to the device-backed mirrors."""


def patch_gpry():
    """After this call ``gpry.Runner`` builds / accepts the MI355X classes.

    Rebinds the names that ``gpry/run.py`` looks up (``GaussianProcessRegressor`` at
    :308,346; acquisition classes by name at :392 -- ``NORA`` and ``BatchOptimizer``;
    ``GenericGPAcquisition`` at :360; the default pre-processors at :318-319).  Returns
    the patched ``gpry`` module.
    """
    import gpry
    import gpry.gpr
    import gpry.gp_acquisition
    import gpry.run
    from gpry_amd.gp_acquisition import NORA, BatchOptimizer, GenericGPAcquisition
    from gpry_amd.gpr import GaussianProcessRegressor
    from gpry_amd.preprocessing import Normalize_bounds, Normalize_y

    gpry.gpr.GaussianProcessRegressor = GaussianProcessRegressor
    gpry.run.GaussianProcessRegressor = GaussianProcessRegressor
    gpry.gp_acquisition.NORA = NORA
    gpry.gp_acquisition.BatchOptimizer = BatchOptimizer
    gpry.run.GenericGPAcquisition = GenericGPAcquisition
    gpry.run.Normalize_bounds = Normalize_bounds
    gpry.run.Normalize_y = Normalize_y
    return gpry


def patch_gpry_mc():
    """Opt-in: after this call ``gpry.mc.mc_sample_from_gp_ns`` is the device nested sampler
    (``gpry_amd.mc.mc_sample_from_gp_ns``), so an unmodified ``Runner.generate_mc_sample()`` -- its "nested" default,
    gpry/run.py:1655-1681 -- samples the surrogate on the device.  The Runner's "mcmc" branch builds Cobaya objects and is
    not rebound; call ``gpry_amd.mc.mc_sample_from_gp(gpr, sampler="mcmc")`` for the device MCMC instead.  Returns the
    patched ``gpry.mc`` module."""
    import gpry.mc
    from gpry_amd.mc import mc_sample_from_gp_ns

    gpry.mc.mc_sample_from_gp_ns = mc_sample_from_gp_ns
    return gpry.mc
