"""Epoch driver over the device-side components -- an original, minimal loop, NOT a copy of the
reference's control plane.

The reference's driver (``models/handler.py``) is out of scope; what the hot path needs either side of it
are four device components, and this module only strings them together:

    ForecastDataset / WindowLoader   resident [T,N] series, index batches        forecast_dataloader.py
    engine.TrainStep                 gather -> fwd -> MSE -> bwd -> optimizer     one hipGraph per step
    ops.roll_window                  rolling multi-step inference                 csrc/data.hip
    math_utils.Scores                de-normalise + MAPE / MAE / RMSE             csrc/data.hip

Two ways to use it:
  * ``DeviceTrainer(...).fit(train_series, valid_series, epochs)`` / ``.evaluate(series)`` -- the native API;
  * ``train(train_data, valid_data, args, result_dir)`` / ``test(test_data, args, train_dir, test_dir)`` -- adapters with
    the call shape ``main.py`` uses (main.py:5,54,60), so the reference's entry script can drive the device loop by
    importing these two names instead of ``models.handler``'s.  Checkpoints use the reference's file names
    (``<epoch>_stemgnn.pt``, best model ``_stemgnn.pt``, whole-module pickles) so they interchange.
The unmodified reference driver also works on top of ``stemgnn_amd.Model`` alone.
"""
import json
import pathlib
import time

import numpy as np
import torch

from . import ops
from .base_model import Model, check_quantiles, point_index
from .engine import ForecastStep, QuantileForecastStep, TrainStep, scenario_rounds
from .forecast_dataloader import ForecastDataset, WindowLoader, denorm_coefficients, mark_missing
from .math_utils import (ConformalCalibrator, EnsembleScores, EnvelopeCalibrator, EventSpec, PathEnvelope, QuantileScores,
                         ScenarioEvents, ScenarioSet, ScenarioTree, Scores, reduce_scenarios, scenario_tree, simultaneous_bands)
from .optim import FusedAdam, FusedRMSprop

BEST = "_stemgnn.pt"
CONFORMAL = "conformal.pt"      # the calibrator fitted on the best model's validation pass, beside the best checkpoint


def checkpoint_path(directory, tag=None):
    """The reference's file names (models/handler.py:21-22: ``str(epoch) if epoch else ''``): the snapshot of epoch 0
    shares the best-model slot ``_stemgnn.pt`` there, so a reference loader finds a model after a one-epoch run without
    validation; kept identical so the files interchange."""
    return pathlib.Path(directory) / (f"{tag}{BEST}" if tag else BEST)


def save_checkpoint(model, directory, tag=None):
    path = checkpoint_path(directory, tag)
    path.parent.mkdir(parents=True, exist_ok=True)
    torch.save(model, path)
    return path


def load_checkpoint(directory, tag=None):
    path = checkpoint_path(directory, tag)
    return torch.load(path, weights_only=False) if path.is_file() else None


def save_calibrator(calibrator, directory):
    path = pathlib.Path(directory) / CONFORMAL
    path.parent.mkdir(parents=True, exist_ok=True)
    torch.save(calibrator.state_dict(), path)
    return path


def load_calibrator(directory, device=None):
    """The ConformalCalibrator saved beside the best checkpoint, or None when the run was not calibrated."""
    path = pathlib.Path(directory) / CONFORMAL
    if not path.is_file():
        return None
    return ConformalCalibrator.from_state_dict(torch.load(path, weights_only=False), device)


def rolling_forecast(model, loader, horizon, adjacency=None):
    """Multi-step forecast of every window the loader yields: the model's first outputs are fed back as inputs until
    `horizon` steps exist (what the reference's validation does, models/handler.py:41-65), all on the device.
    adjacency (a graph.LatentGraph or an [N,N] tensor): every round is ``model.predict(window, adjacency=adjacency)`` -- the
    forecast from a fixed graph, independent of how the loader batches the windows.
    Returns (forecast [count, horizon, N], target [count, horizon, N]) float32 device tensors.
    A quantile model (``model.quantiles``): the POINT row (``model.point_index``) is what is fed back as the next window, and the
    forecast comes back as [count, Q, horizon, N] (``ops.roll_window_quantile``).  With `horizon` beyond the model's own, the
    bands of the later rounds are therefore conditional on the point path: they describe the spread around a forecast made
    from the model's own median-like outputs, not the wider uncertainty of the inputs those rounds never saw
    (rolling_scenarios rolls sampled paths and reads those bands off them)."""
    quantiles = getattr(model, "quantiles", None)
    was_training = model.training
    model.eval()
    forecasts, targets = [], []
    with torch.no_grad():
        for window, target in loader:
            if quantiles is None:
                steps = torch.zeros(window.shape[0], horizon, window.shape[2], device=window.device)
            else:
                steps = torch.zeros(window.shape[0], len(quantiles), horizon, window.shape[2], device=window.device)
            done = 0
            while done < horizon:
                out, _ = model(window) if adjacency is None else model.predict(window, adjacency=adjacency)
                if out.shape[-2] == 0:
                    raise Exception("Get blank inference result")
                if quantiles is None:
                    window = ops.roll_window(window, out, steps, done, horizon)
                else:
                    window = ops.roll_window_quantile(window, out, steps, done, horizon, model.point_index)
                done += min(horizon - done, out.shape[-2])
            forecasts.append(steps)
            targets.append(target)
    model.train(was_training)
    return torch.cat(forecasts), torch.cat(targets)


def _check_scenarios(who, model, horizon, paths):
    quantiles = getattr(model, "quantiles", None)
    if quantiles is None or len(quantiles) < 2:
        raise ValueError(f"{who} needs a quantile model with at least two levels (Model(..., quantiles=...)): a point "
                         "model has no quantile function to draw from")
    if int(horizon) < 1 or not 1 <= int(paths) <= 1024:
        raise ValueError(f"{who}: horizon must be at least 1 and paths within [1, 1024], got {horizon}, {paths}")


def rolling_scenarios(model, loader, horizon, paths=64, seed=0, adjacency=None, coupling="independent", tails="linear",
                      return_paths=False, origin=0, events=None):
    """Multi-step forecast of every window the loader yields from SAMPLED trajectories: where rolling_forecast feeds the point
    row back, each of `paths` trajectories per window draws its next rows from the predicted quantile function (the piecewise-
    linear one through the model's levels and rearranged rows: ops.scenario_roll) and the model runs on all of them as one
    batch.  The bands of the first round (the model's own horizon L) are the model's rows, rolling_forecast's bit for bit;
    the bands of the later steps are order statistics of the paths (ops.scenario_bands), so they carry the uncertainty of
    the inputs those rounds never saw.
    Per loader batch of Bo windows: one predict on the windows, then ceil(horizon / L) - 1 predicts at batch Bo * paths.
    coupling: "independent" draws every (step, node) on its own, "path" moves all nodes of a path and round with one uniform;
    the two bracket the real dependence between nodes.  tails: "linear" extends the outermost segments of the quantile
    function beyond the outer levels, "clamp" stops at them.  seed: the Philox key; origin: the global index of the loader's
    first window.  The origin index runs on over the batches, so a window's draws do not depend on how the loader batches it;
    with adjacency= (as in rolling_forecast) nor does anything else.  Without adjacency= the latent graph of a round is the
    mean over all paths of the batch.
    Returns (bands [count, Q, horizon, N], target [count, horizon, N]) and, with return_paths, paths [count, S, horizon, N],
    float32 device tensors in the forecast's normalised units: ConformalCalibrator.fit and QuantileScores take them as they are.
    A calibrator fitted on point-path bands (rolling_forecast's) is not valid for these bands.  The model's training state is
    restored on exit.
    events (a math_utils.EventSpec): every loader batch's paths are counted as they are produced (`events.count`) and the joined
    math_utils.ScenarioEvents is returned as the LAST element of the tuple -- a pass no longer has to keep its paths to ask
    about them; return_paths is still honoured.  Without the keyword the function is call for call what it was."""
    _check_scenarios("rolling_scenarios", model, horizon, paths)
    bands, targets, trajectories, counted = [], [], [], []
    for b, target, p in _scenario_batches(model, loader, horizon, paths, seed, adjacency, coupling, tails, origin):
        bands.append(b)
        targets.append(target)
        if return_paths:
            trajectories.append(p)
        if events is not None:
            counted.append(events.count(p))
    out = (torch.cat(bands), torch.cat(targets)) + ((torch.cat(trajectories),) if return_paths else ())
    return out if events is None else out + (ScenarioEvents.cat(counted),)


def _scenario_batches(model, loader, horizon, paths, seed, adjacency, coupling, tails, origin):
    """The batch loop of rolling_scenarios and reduced_scenarios: yields (bands [Bo,Q,horizon,N], target, paths [Bo,S,horizon,N])
    per loader batch, the origin index running on over the batches; the model is in eval mode while the loop runs and gets its
    training state back when it ends, however it ends."""
    horizon, paths = int(horizon), int(paths)
    graph_kw = {} if adjacency is None else dict(adjacency=adjacency)
    was_training = getattr(model, "training", False)
    model.eval()
    count = int(origin)
    try:
        with torch.no_grad():
            for window, target in loader:
                b, p = scenario_rounds(model, window, horizon, paths, count, seed, coupling, tails, graph_kw)
                count += window.shape[0]
                yield b, target, p
    finally:
        model.train(was_training)


def reduced_scenarios(model, loader, horizon, keep, paths=64, seed=0, adjacency=None, coupling="independent", tails="linear",
                      origin=0, on=None, scale=None, squared=False):
    """rolling_scenarios handing on `keep` representative paths with probabilities per window instead of `paths` equally likely
    ones: every loader batch's paths are reduced as they are produced (math_utils.reduce_scenarios: forward selection on the
    distance between whole trajectories), so the pass keeps count * keep paths, not count * paths.  The arguments up to `origin`
    are rolling_scenarios'; on / scale / squared are reduce_scenarios' (on: an EventSpec with groups=, whose aggregate of every
    batch's paths the distances are taken on; a tensor cannot be named ahead of the paths).
    Returns (bands, target, math_utils.ScenarioSet): the bands and the target are rolling_scenarios' own, and the set is
    `reduce_scenarios(paths, keep, ...)` of rolling_scenarios(..., return_paths=True)'s paths, bit for bit, however the loader
    batches the windows.  The set keeps neither the distances nor the full paths: its head(k) needs one of them put back."""
    _check_scenarios("reduced_scenarios", model, horizon, paths)
    if on is not None and not isinstance(on, EventSpec):
        raise ValueError("reduced_scenarios: on= is an EventSpec with groups= (the aggregate of every batch's paths); a tensor "
                         "goes to math_utils.reduce_scenarios with the paths it belongs to")
    bands, targets, sets = [], [], []
    for b, target, p in _scenario_batches(model, loader, horizon, paths, seed, adjacency, coupling, tails, origin):
        bands.append(b)
        targets.append(target)
        kept = reduce_scenarios(p, keep, on=on, scale=scale, squared=squared)
        kept.source = None                                   # the batch's paths go with the batch
        sets.append(kept)
    return torch.cat(bands), torch.cat(targets), ScenarioSet.cat(sets)


def scenario_trees(model, loader, horizon, stages, nodes, paths=64, seed=0, adjacency=None, coupling="independent",
                   tails="linear", origin=0, on=None, scale=None, squared=False):
    """rolling_scenarios handing on a scenario tree per window instead of `paths` equally likely ones: every loader batch's
    paths become a tree as they are produced (math_utils.scenario_tree: staged forward selection, the members of a node
    sharing their history up to the stage's bound), and the batch's paths are dropped.  The arguments up to `origin` are
    rolling_scenarios'; stages / nodes / on / scale / squared are scenario_tree's (on: an EventSpec with groups=).
    Returns (bands, target, math_utils.ScenarioTree): the bands and the target are rolling_scenarios' own, and the tree is
    `scenario_tree(paths, stages, nodes, ...)` of rolling_scenarios(..., return_paths=True)'s paths, bit for bit, however the
    loader batches the windows."""
    _check_scenarios("scenario_trees", model, horizon, paths)
    if on is not None and not isinstance(on, EventSpec):
        raise ValueError("scenario_trees: on= is an EventSpec with groups= (the aggregate of every batch's paths); a tensor "
                         "goes to math_utils.scenario_tree with the paths it belongs to")
    bands, targets, trees = [], [], []
    for b, target, p in _scenario_batches(model, loader, horizon, paths, seed, adjacency, coupling, tails, origin):
        bands.append(b)
        targets.append(target)
        trees.append(scenario_tree(p, stages, nodes, on=on, scale=scale, squared=squared))
    return torch.cat(bands), torch.cat(targets), ScenarioTree.cat(trees)


def scenario_envelopes(model, loader, horizon, coverage=0.9, paths=64, seed=0, adjacency=None, coupling="independent",
                       tails="linear", origin=0, on=None, calibrator=None, ignore_nan=False):
    """rolling_scenarios handing on the simultaneous band of every window instead of its `paths` trajectories: every loader
    batch's paths are enveloped against that batch's target as they are produced (math_utils.simultaneous_bands: a centre and a
    scale per step and one multiplier, so that the WHOLE trajectory stays inside), then dropped.  The arguments up to `origin`
    are rolling_scenarios'; coverage / on / calibrator / ignore_nan are simultaneous_bands' (on: an EventSpec with groups=,
    whose aggregate of every batch's paths and target the band is made for).
    Returns (bands, target, math_utils.PathEnvelope): the bands and the target are rolling_scenarios' own, and the envelope is
    `simultaneous_bands(paths, coverage, target=target, ...)` of rolling_scenarios(..., return_paths=True)'s paths, bit for
    bit, however the loader batches the windows.  Its `truth` from a held-out pass is what EnvelopeCalibrator.fit takes."""
    _check_scenarios("scenario_envelopes", model, horizon, paths)
    if on is not None and not isinstance(on, EventSpec):
        raise ValueError("scenario_envelopes: on= is an EventSpec with groups= (the aggregate of every batch's paths); a tensor "
                         "goes to math_utils.simultaneous_bands with the paths it belongs to")
    bands, targets, envelopes = [], [], []
    for b, target, p in _scenario_batches(model, loader, horizon, paths, seed, adjacency, coupling, tails, origin):
        bands.append(b)
        targets.append(target)
        envelopes.append(simultaneous_bands(p, coverage, on=on, target=target, calibrator=calibrator, ignore_nan=ignore_nan))
    return torch.cat(bands), torch.cat(targets), PathEnvelope.cat(envelopes)


def rolling_forecast_graph(model, dataset, horizon, batch_size, adjacency=None):
    """rolling_forecast(model, WindowLoader(dataset, batch_size), horizon) on engine.ForecastStep: each full batch is one
    hipGraph replay of window gather -> Model.predict -> roll_window rounds -> result slabs; the ragged last batch runs
    eagerly.  Same (forecast, target) [count, horizon, N], bit for bit; the model's training state is left untouched.
    The dataset's horizon (its target length) must equal `horizon`.  adjacency: as in rolling_forecast."""
    if getattr(model, "quantiles", None) is not None:
        raise ValueError("rolling_forecast_graph does not take a quantile model (engine.ForecastStep's result slabs hold one "
                         "[H,N] forecast per window); use rolling_quantile_forecast_graph")
    if int(dataset.horizon) != int(horizon):
        raise ValueError(f"rolling_forecast_graph: dataset horizon {dataset.horizon} != horizon {horizon}")
    n = len(dataset)
    step = ForecastStep(model, batch_size, dataset.window_size, horizon, dataset.data, order_capacity=n, adjacency=adjacency)
    step.load_order(dataset.hi_all)
    while step.remaining > 0:
        step.run_next()
    return step.result()


def rolling_quantile_forecast_graph(model, dataset, horizon, batch_size, adjacency=None, rearrange=False, calibrator=None):
    """rolling_forecast of a quantile model on engine.QuantileForecastStep: each full batch is one hipGraph replay of window
    gather -> Model.predict -> roll_window_quantile rounds -> ONE quantile_store into the result slabs; the ragged last batch
    runs eagerly.  Returns (forecast [count, Q, horizon, N], target [count, horizon, N]).
    rearrange: every (window, step, node)'s Q values leave the graph in non-decreasing order (math_utils.rearrange_quantiles);
    calibrator (a fitted math_utils.ConformalCalibrator): its offsets are applied to the (rearranged) rows -- with rearrange on
    it must have been fitted on rearranged forecasts.  With both off the result is rolling_forecast's, bit for bit; with them
    it is ``calibrator.apply(torch.sort(forecast, dim=1, stable=True).values)`` of that, bit for bit.  Neither touches the window
    that is fed back.  The dataset's horizon must equal `horizon`; adjacency: as in rolling_forecast."""
    if int(dataset.horizon) != int(horizon):
        raise ValueError(f"rolling_quantile_forecast_graph: dataset horizon {dataset.horizon} != horizon {horizon}")
    n = len(dataset)
    step = QuantileForecastStep(model, batch_size, dataset.window_size, horizon, dataset.data, order_capacity=n,
                                adjacency=adjacency, rearrange=rearrange, calibrator=calibrator)
    step.load_order(dataset.hi_all)
    while step.remaining > 0:
        step.run_next()
    return step.result()


def score_forecast(forecast, target, norm_method=None, statistic=None, dump_dir=None, ignore_nan=False, quantiles=None,
                   calibrator=None, origin=None, paths=None, fair=False, envelope=None, events=None):
    """Metrics of a rolling forecast in raw units (and normalised units under ``*_norm``).  With `dump_dir`, the first
    forecast step of every window is written as CSV (target / predict / absolute error / absolute percentage error).
    ignore_nan: NaN targets (missing readings) are left out of every metric; the CSV files keep them as NaN.
    A 4-D forecast [count, Q, horizon, N] needs `quantiles` (the Q levels): every key above is computed from the point row
    (the level closest to 0.5) through the same metrics kernel, and the calibration of the bands is added in raw units
    (math_utils.QuantileScores): ``pinball`` (mean over the levels), ``pinball_q`` / ``coverage_q`` [Q], ``interval_coverage`` /
    ``interval_width`` / ``interval_nominal`` [Q // 2] for the pairs (i, Q-1-i), and ``crossing``.
    calibrator (a fitted math_utils.ConformalCalibrator): the bands are calibrated, in the forecast's normalised units, ahead of
    those figures, and the uncalibrated ones are kept under ``interval_coverage_raw`` / ``interval_width_raw``; the point row and
    every point metric are untouched.  A math_utils.SeasonalConformalCalibrator also needs `origin`, the time index of every
    window's step-0 target (an int: window i has origin + i; or an int64 tensor [count]).
    paths [count, S, horizon, N] (rolling_scenarios(..., return_paths=True)): the sampled trajectories are scored as an ensemble
    (math_utils.EnsembleScores; `fair` is its flag): ``crps``, ``energy_score``, ``ensemble_rmse``, ``spread`` and
    ``rank_histogram`` [S + 1], each also per step under ``*_step``, in raw units and, like the keys above, in normalised
    units under ``*_norm`` (the histogram has no units).  Without paths= the result is what it was, key for key.
    paths a math_utils.ScenarioSet (reduced_scenarios' third result): its kept paths are scored with their weights
    (ScenarioSet.scores; the histogram has total + 1 bins), and events= counts them with their weights.
    events (a math_utils.EventSpec; needs paths=): the event's odds read off the paths are verified against the target
    (math_utils.EventScores; the spec's own threshold, groups and mul / add): ``event_brier``, ``event_brier_skill``,
    ``event_base_rate`` and ``event_reliability`` [M, S + 1, 2] for "the event at some step", the same under ``*_run`` for "at
    least min_run steps in a row" and under ``*_step`` ([horizon], the table [horizon, M, S + 1, 2]) for every single step;
    ignore_nan leaves the (origin, column) pairs with a missing target out.  Without events= the keys are what they were.
    envelope (a coverage inside (0, 1), or a fitted math_utils.EnvelopeCalibrator; needs paths= and a quantile forecast): the
    simultaneous band of the paths (math_utils.simultaneous_bands) is verified against the target: ``joint_coverage``, the share
    of (window, node) pairs whose whole trajectory the band holds; ``joint_coverage_pointwise``, the same share for the outer
    pair of the forecast's own (calibrated) bands; ``envelope_width`` [horizon], the band's mean width per step in raw units.
    Both shares are taken over the same pairs, those with a truth depth: a pair with a NaN target step is left out of both
    (with ignore_nan only its NaN steps are, and a pair without any step), and so is an absent column of the envelope.
    Without envelope= the keys are what they were."""
    if events is not None and paths is None:
        raise ValueError("score_forecast: events= goes with paths= (the sampled trajectories the odds are read from)")
    if envelope is not None and (paths is None or forecast.dim() != 4):
        raise ValueError("score_forecast: envelope= goes with paths= (the sampled trajectories the band is made from) and a "
                         "[count, Q, horizon, N] forecast")
    seasonal = getattr(calibrator, "kind", None) == "seasonal"
    if seasonal and origin is None:
        raise ValueError("score_forecast: a seasonal calibrator needs origin= (the time index of every window's first target)")
    if origin is not None and not seasonal:
        raise ValueError("score_forecast: origin= goes with a seasonal calibrator")
    mul = add = None
    if norm_method and statistic:
        mul, add = denorm_coefficients(norm_method, statistic, forecast.device)
    calibration = {}
    if forecast.dim() == 4:
        if quantiles is None:
            raise ValueError("score_forecast: a [count, Q, horizon, N] forecast needs quantiles=")
        quantiles = check_quantiles(quantiles)
        if forecast.shape[1] != len(quantiles):
            raise ValueError(f"score_forecast: forecast has {forecast.shape[1]} quantile rows, quantiles= names {len(quantiles)}")
        raw_bands = {}
        if calibrator is not None:
            qs = QuantileScores(target, forecast, quantiles, mul, add, ignore_nan=ignore_nan)
            raw_bands = dict(interval_coverage_raw=qs.interval_coverage, interval_width_raw=qs.interval_width)
            point_row = forecast[:, point_index(quantiles)].contiguous()
            forecast = calibrator.apply(forecast, origin) if seasonal else calibrator.apply(forecast)
        qs = QuantileScores(target, forecast, quantiles, mul, add, ignore_nan=ignore_nan)
        calibration = dict(pinball=float(qs.pinball.mean()), pinball_q=qs.pinball, coverage_q=qs.coverage,
                           interval_coverage=qs.interval_coverage, interval_width=qs.interval_width,
                           interval_nominal=qs.interval_nominal, crossing=float(qs.crossing), **raw_bands)
        outer = (forecast[:, 0], forecast[:, -1])
        forecast = point_row if calibrator is not None else forecast[:, point_index(quantiles)].contiguous()
    elif quantiles is not None:
        raise ValueError("score_forecast: quantiles= goes with a [count, Q, horizon, N] forecast")
    elif calibrator is not None:
        raise ValueError("score_forecast: calibrator= goes with a [count, Q, horizon, N] forecast")
    raw = Scores(target, forecast, mul, add, ignore_nan=ignore_nan)
    (mape, mae, rmse), (mape_n, mae_n, rmse_n) = raw.get(), raw.get(by_node=True)
    out = dict(mae=mae, mape=mape, rmse=rmse, mae_node=mae_n, mape_node=mape_n, rmse_node=rmse_n)
    normed = Scores(target, forecast, ignore_nan=ignore_nan).get() if mul is not None else (mape, mae, rmse)
    out.update(mape_norm=normed[0], mae_norm=normed[1], rmse_norm=normed[2])
    out.update(calibration)
    if paths is not None:
        if isinstance(paths, ScenarioSet):                   # the kept paths with their weights: the same keys, total + 1 bins
            ens = paths.scores(target, mul, add, ignore_nan=ignore_nan, fair=fair)
            ens_n = paths.scores(target, ignore_nan=ignore_nan, fair=fair) if mul is not None else ens
        else:
            ens = EnsembleScores(target, paths, mul, add, ignore_nan=ignore_nan, fair=fair)
            ens_n = EnsembleScores(target, paths, ignore_nan=ignore_nan, fair=fair) if mul is not None else ens
        for key, name in (("crps", "crps"), ("energy_score", "energy"), ("ensemble_rmse", "rmse"), ("spread", "spread")):
            for suffix in ("", "_step"):
                out[key + suffix] = getattr(ens, name + suffix)
                out[key + suffix + "_norm"] = getattr(ens_n, name + suffix)
        out.update(rank_histogram=ens.rank_histogram, rank_histogram_step=ens.rank_histogram_step)
    if events is not None:
        sc = events.count(paths).score(events.realised(target), ignore_nan=ignore_nan)
        for suffix in ("", "_run", "_step"):
            out["event_brier" + suffix] = getattr(sc, "brier" + suffix)
            out["event_brier_skill" + suffix] = getattr(sc, "skill" + suffix)
            out["event_base_rate" + suffix] = getattr(sc, "base_rate" + suffix)
            out["event_reliability" + suffix] = getattr(sc, "reliability" + suffix)
    if envelope is not None:
        fitted = envelope if isinstance(envelope, EnvelopeCalibrator) else None
        env = simultaneous_bands(paths, fitted.coverage if fitted is not None else envelope, target=target, calibrator=fitted,
                                 ignore_nan=ignore_nan)
        width = env.bands[:, 1].double() - env.bands[:, 0].double()
        if mul is not None:
            width = width * mul
        y = target.double()                                  # the pointwise band over the pairs the envelope is judged on
        judged = ~torch.isnan(env.truth)
        held = (((y >= outer[0].double()) & (y <= outer[1].double())) | torch.isnan(y)).all(dim=1) & judged
        both = torch.stack([held.sum(), judged.sum()]).cpu()
        out.update(joint_coverage=env.joint_coverage()[0],
                   joint_coverage_pointwise=float(both[0]) / float(both[1]) if int(both[1]) else float("nan"),
                   envelope_width=torch.nanmean(width.transpose(0, 1).reshape(width.shape[1], -1), dim=1).cpu().numpy())
    if dump_dir is not None:
        d = pathlib.Path(dump_dir)
        d.mkdir(parents=True, exist_ok=True)
        pred, true = forecast[:, 0, :].double(), target[:, 0, :].double()
        if mul is not None:
            pred, true = pred * mul + add, true * mul + add
        pred, true = pred.cpu().numpy(), true.cpu().numpy()
        err = np.abs(pred - true)
        with np.errstate(divide="ignore", invalid="ignore"):
            ape = err / np.abs(true)
        for name, arr in (("target", true), ("predict", pred), ("predict_abs_error", err), ("predict_ape", ape)):
            np.savetxt(d / f"{name}.csv", arr, delimiter=",")
    return out


def column_statistics(series, norm_method, missing=None):
    """missing (see ForecastDataset): the statistics are taken over the valid entries of every column only."""
    series = np.asarray(series)
    mean, std, lo, hi = np.mean, np.std, np.min, np.max
    if missing is not None:
        series, _ = mark_missing(series, missing)
        mean, std, lo, hi = np.nanmean, np.nanstd, np.nanmin, np.nanmax
    if norm_method == "z_score":
        return {"mean": mean(series, axis=0).tolist(), "std": std(series, axis=0).tolist()}
    if norm_method == "min_max":
        return {"min": lo(series, axis=0).tolist(), "max": hi(series, axis=0).tolist()}
    return None


class DeviceTrainer:
    """Owns model + optimizer + LR schedule; `fit` runs epochs of hipGraph train steps with validation in between."""

    def __init__(self, units, window, horizon, multi, *, batch_size=32, lr=1e-4, optimizer="RMSProp", decay_rate=0.5,
                 decay_every=5, norm_method="z_score", device="cuda", model_factory=None, hipgraph=True,
                 dropout_seed=None, weight_decay=0.0, max_grad_norm=None, skip_nonfinite=False, loss="mse", huber_delta=1.0,
                 missing=None, quantiles=None, calibrate=False, calibrate_per_step=True, calibrate_per_node=False):
        """loss / huber_delta: the training loss of engine.TrainStep ("mse" | "mae" | "huber").  quantiles (levels in (0, 1),
        increasing): a quantile model (Model(..., quantiles=); a `model_factory` gets the keyword too) trained by the pinball loss
        -- `loss` left at its default means "pinball" then; validation keeps selecting the best model on the point forecast's
        MAE and prints the bands' coverage beside it.  missing (a float, e.g. 0.0):
        raw NaN entries and entries equal to it are missing readings -- left out of the column statistics, the training loss
        and the validation metrics, while the model's inputs stay imputed (ForecastDataset).
        calibrate (a quantile model only): whenever validation finds a new best model, a math_utils.ConformalCalibrator
        (calibrate_per_step / calibrate_per_node: its grouping) is fitted from that pass's forecast and target, kept as
        `self.calibrator` and saved beside the best checkpoint as ``conformal.pt``; trainer.test applies it."""
        self.units, self.window, self.horizon, self.multi = units, window, horizon, multi
        self.batch_size, self.norm_method, self.device, self.hipgraph = batch_size, norm_method, device, hipgraph
        self.decay_every = decay_every
        self.quantiles = None if quantiles is None else check_quantiles(quantiles)
        if self.quantiles is not None and loss == "mse":
            loss = "pinball"
        self.loss, self.huber_delta, self.missing = loss, huber_delta, missing
        if calibrate and (self.quantiles is None or len(self.quantiles) < 2):
            raise ValueError("DeviceTrainer: calibrate=True needs a quantile model with at least two levels (quantiles=)")
        self.calibrate = bool(calibrate)
        self.calibrate_per_step, self.calibrate_per_node = bool(calibrate_per_step), bool(calibrate_per_node)
        self.calibrator = None
        self._last_pass = None
        head = {} if self.quantiles is None else dict(quantiles=self.quantiles)
        self.model = (model_factory or Model)(units, 2, window, multi, horizon=horizon, **head)
        self.model.to(device)
        if dropout_seed is not None and hasattr(self.model, "set_dropout_seed"):
            # an explicit Philox key for the attention dropout: by default the key follows the device generator's seed AND
            # the model's construction index in this process (two models never share a mask stream), so a run is only
            # reproducible if models are built in the same order; naming the key removes that dependence
            self.model.set_dropout_seed(int(dropout_seed), 0, torch.device(device))
        # gradient-norm clipping / weight decay / non-finite skip inside the fused step (optim.py); defaults: the step as it was
        controls = dict(weight_decay=weight_decay, max_grad_norm=max_grad_norm, skip_nonfinite=skip_nonfinite)
        if optimizer == "RMSProp":
            self.optimizer = FusedRMSprop(self.model.parameters(), lr=lr, eps=1e-8, **controls)
        else:                                   # the driver's other branch (models/handler.py:128-129), fused as well
            self.optimizer = FusedAdam(self.model.parameters(), lr=lr, betas=(0.9, 0.999), **controls)
        self.schedule = torch.optim.lr_scheduler.ExponentialLR(self.optimizer, gamma=decay_rate)
        self.statistic = None
        self.stepper = None

    def _dataset(self, series):
        return ForecastDataset(series, window_size=self.window, horizon=self.horizon, normalize_method=self.norm_method,
                               norm_statistic=self.statistic, device=self.device, missing=self.missing)

    def validate(self, loader, dump_dir=None):
        forecast, target = rolling_forecast(self.model, loader, self.horizon)
        if self.calibrate:
            self._last_pass = (forecast, target)      # what fit() calibrates from when this pass is the best one so far
        return score_forecast(forecast, target, self.norm_method, self.statistic, dump_dir,
                              ignore_nan=self.missing is not None, quantiles=self.quantiles)

    def _calibrate_from_last_pass(self, out_dir=None):
        forecast, target = self._last_pass
        self.calibrator = ConformalCalibrator(self.quantiles, self.calibrate_per_step, self.calibrate_per_node)
        self.calibrator.fit(target, forecast, ignore_nan=self.missing is not None)
        if out_dir is not None:
            save_calibrator(self.calibrator, out_dir)
        return self.calibrator

    def fit(self, train_series, valid_series, epochs, *, validate_every=1, patience=None, out_dir=None, on_step=None,
            on_validate=None, log=print):
        if len(train_series) == 0:
            raise Exception("Cannot organize enough training data")
        if len(valid_series) == 0:
            raise Exception("Cannot organize enough validation data")
        self.statistic = column_statistics(train_series, self.norm_method, self.missing)
        if out_dir is not None and self.statistic is not None:
            pathlib.Path(out_dir).mkdir(parents=True, exist_ok=True)
            (pathlib.Path(out_dir) / "norm_stat.json").write_text(json.dumps(self.statistic))
        train_set, valid_set = self._dataset(train_series), self._dataset(valid_series)
        batches = WindowLoader(train_set, batch_size=self.batch_size, drop_last=False, shuffle=True)
        valid_loader = WindowLoader(valid_set, batch_size=self.batch_size, shuffle=False)
        log(f"trainable parameters: {sum(p.numel() for p in self.model.parameters() if p.requires_grad)}")
        self.stepper = TrainStep(self.model, self.optimizer, self.batch_size, self.window, self.horizon, self.units,
                                 series=train_set.data, graph=self.hipgraph, order_capacity=len(train_set), loss=self.loss,
                                 huber_delta=self.huber_delta, ignore_nan=self.missing is not None,
                                 target_series=train_set.target)
        best, stale, metrics = float("inf"), 0, {}
        for epoch in range(epochs):
            t0 = time.time()
            self.model.train()
            n_steps = 0
            # the epoch's shuffled order goes to the device-side iterator once; full batches are then one graph replay
            # each (TrainStep.run_next), the ragged last batch (drop_last=False, handler.py:136) runs eagerly
            epoch_batches = list(batches.index_batches())
            full = [idx for idx in epoch_batches if idx.numel() == self.batch_size]
            if full:
                self.stepper.load_order(train_set.hi_all.index_select(0, torch.cat(full)))
            for i, idx in enumerate(epoch_batches):
                if idx.numel() == self.batch_size:
                    self.stepper.run_next()
                else:
                    self.stepper.run_indices(train_set.hi_all.index_select(0, idx))
                n_steps += 1
                if on_step is not None:
                    on_step(epoch, i, self.stepper)
            mean_loss = self.stepper.epoch_loss_sum() / max(n_steps, 1)       # one host sync per epoch
            ops.check_gather_status(train_set.device)                       # both raise if a device-side check tripped
            ops.check_gru_status(train_set.device)
            controls = ""
            if self.optimizer.controls_enabled:                             # one more host sync per epoch, only then
                rep = self.optimizer.grad_report(reset=True)
                controls = f"  clipped {rep['clipped_steps']}/{n_steps}, skipped {rep['skipped_steps']}"
            log(f"epoch {epoch}: {time.time() - t0:.2f}s  mean train loss {mean_loss:.4f}{controls}  [{self.stepper.mode}]")
            if out_dir is not None:
                save_checkpoint(self.model, out_dir, epoch)
            if (epoch + 1) % self.decay_every == 0:
                self.schedule.step()
            if (epoch + 1) % validate_every == 0:
                metrics = self.validate(valid_loader, out_dir)
                ops.check_gru_status(train_set.device)
                log(f"  validation: MAPE {metrics['mape']:.6%}  MAE {metrics['mae']:.6f}  RMSE {metrics['rmse']:.6f}"
                    f"  (normalised MAE {metrics['mae_norm']:.6f})")
                if self.quantiles is not None:
                    bands = "  ".join(f"{c:.1%} of {n:.0%}" for c, n in
                                      zip(metrics["interval_coverage"], metrics["interval_nominal"]))
                    log(f"  quantiles: pinball {metrics['pinball']:.6f}  coverage "
                        + " ".join(f"{t:g}:{c:.1%}" for t, c in zip(self.quantiles, metrics["coverage_q"]))
                        + (f"  intervals {bands}" if bands else "") + f"  crossing {metrics['crossing']:.2%}")
                if on_validate is not None:
                    on_validate(epoch, metrics)
                if metrics["mae"] < best:
                    best, stale = metrics["mae"], 0
                    if out_dir is not None:
                        save_checkpoint(self.model, out_dir)
                    if self.calibrate:
                        cal = self._calibrate_from_last_pass(out_dir)
                        log("  conformal: offsets per pair "
                            + "  ".join(f"{n:.0%}: {float(o.min()):+.4f} .. {float(o.max()):+.4f}"
                                        for n, o in zip(cal.interval_nominal, cal.offsets))
                            + f"  ({int(cal.offsets[0].numel())} group(s) per pair, normalised units)")
                else:
                    stale += 1
            if patience is not None and stale >= patience:
                break
        self._last_pass = None
        return metrics, self.statistic

    def evaluate(self, series, dump_dir=None):
        loader = WindowLoader(self._dataset(series), batch_size=self.batch_size, drop_last=False, shuffle=False)
        return self.validate(loader, dump_dir)


# ---- adapters with main.py's call shape (main.py:54, :60) -----------------------------------------------------------
def train(train_data, valid_data, args, result_file, model_factory=None, on_step=None, on_validate=None):
    trainer = DeviceTrainer(train_data.shape[1], args.window_size, args.horizon, args.multi_layer,
                            batch_size=args.batch_size, lr=args.lr, optimizer=args.optimizer, decay_rate=args.decay_rate,
                            decay_every=args.exponential_decay_step, norm_method=args.norm_method, device=args.device,
                            model_factory=model_factory, hipgraph=getattr(args, "hipgraph", True),
                            weight_decay=getattr(args, "weight_decay", 0.0), max_grad_norm=getattr(args, "max_grad_norm", None),
                            skip_nonfinite=getattr(args, "skip_nonfinite", False), loss=getattr(args, "loss", "mse"),
                            huber_delta=getattr(args, "huber_delta", 1.0), missing=getattr(args, "missing", None),
                            quantiles=getattr(args, "quantiles", None), calibrate=getattr(args, "calibrate", False),
                            calibrate_per_step=getattr(args, "calibrate_per_step", True),
                            calibrate_per_node=getattr(args, "calibrate_per_node", False))
    patience = getattr(args, "early_stop_step", 10) if getattr(args, "early_stop", False) else None
    return trainer.fit(train_data, valid_data, args.epoch, validate_every=args.validate_freq, patience=patience,
                       out_dir=result_file, on_step=on_step, on_validate=on_validate)


def test(test_data, args, result_train_file, result_test_file):
    model = load_checkpoint(result_train_file)
    if model is None:
        raise FileNotFoundError(f"no best-model checkpoint under {result_train_file}")
    statistic = json.loads((pathlib.Path(result_train_file) / "norm_stat.json").read_text())
    dataset = ForecastDataset(test_data, window_size=args.window_size, horizon=args.horizon,
                              normalize_method=args.norm_method, norm_statistic=statistic, device=args.device)
    loader = WindowLoader(dataset, batch_size=args.batch_size, drop_last=False, shuffle=False)
    forecast, target = rolling_forecast(model, loader, args.horizon)
    quantiles = getattr(model, "quantiles", None)
    calibrator = load_calibrator(result_train_file, forecast.device) if quantiles is not None else None
    metrics = score_forecast(forecast, target, args.norm_method, statistic, result_test_file, quantiles=quantiles,
                             calibrator=calibrator)
    print(f"test: MAPE {metrics['mape']:.4f}  MAE {metrics['mae']:.4f}  RMSE {metrics['rmse']:.4f}")
    if calibrator is not None:
        print("test: interval coverage " + "  ".join(
            f"{n:.0%}: raw {r:.1%} -> calibrated {c:.1%}" for n, r, c in
            zip(metrics["interval_nominal"], metrics["interval_coverage_raw"], metrics["interval_coverage"])))
    return metrics
