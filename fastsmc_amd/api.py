"""Python-facing helpers over the pybind11 module ``_pyasmc`` (the reference's ``asmc`` package surface).

``from fastsmc_amd.api import *`` gives the reference names: ``DecodingParams``, ``DecodingQuantities``,
``Data``, ``HMM``, ``ASMC``, ``FastSMC``, ``DecodingModeOverall``, ``DecodingMode`` ...
"""
from __future__ import annotations

import numpy as np

from . import _pyasmc
from ._pyasmc import (ASMC, BinaryDataReader, Data, DecodePairsReturnStruct, DecodingMode, DecodingModeOverall,  # noqa: F401
                      DecodingParams, DecodingQuantities, DecodingReturnValues, FastSMC, HMM, IbdPairDataLine, Individual,
                      Match, PairObservations, cmBetween, hashingCandidates, hashingCandidatesDevice, hashingWords)

__all__ = ["ASMC", "BinaryDataReader", "IbdPairDataLine", "Data", "DecodePairsReturnStruct", "DecodingMode", "DecodingModeOverall", "DecodingParams",
           "DecodingQuantities", "DecodingReturnValues", "FastSMC", "HMM", "Individual", "PairObservations", "Match", "cmBetween",
           "hashingCandidates", "hashingCandidatesDevice", "hashingWords",
           "decoding_quantities_from_tables", "PreparedModelView", "site_bins", "tail_states", "site_widths", "state_runs"]


def decoding_quantities_from_tables(t) -> DecodingQuantities:
    """Wrap a ``fastsmc_amd.synth.ModelTables`` as a ``DecodingQuantities`` without going through a file."""
    return DecodingQuantities.from_arrays(
        int(t.csfs_samples), t.discretization, t.expected_times, t.initial_state_prob, t.column_ratios, t.keys,
        t.D, t.B, t.U, t.RR, t.compressed_emission, t.classic_emission, t.folded_ascertained_csfs, t.ascertained_csfs,
        t.csfs, t.folded_csfs, t.homozygous_keys if t.homozygous_keys.size else None,
        t.homozygous if t.homozygous_keys.size else None)


class PreparedModelView:
    """Attribute view of ``HMM.preparedModel()`` (the argument ``capi.Context.create_model`` expects)."""

    def __init__(self, d: dict):
        self.__dict__.update(d)
        self.probability_threshold = np.float32(d["probability_threshold"])


def site_bins(positions, width) -> np.ndarray:
    """Bin edges for ``ASMC.decodePairs(..., site_bins=...)`` that cut the sites into windows of ``width``: ``positions``
    are the sites' coordinates in ascending order (cM or bp, any unit ``width`` is in), window ``w`` is
    ``[positions[0] + w * width, positions[0] + (w + 1) * width)``.  Returns int32 edges ``e`` with ``e[0] = 0`` and
    ``e[-1] = len(positions)``; bin ``b`` is sites ``[e[b], e[b + 1])``.  Windows that hold no site are dropped, so the
    edges are strictly ascending (a bin is then one window, never several)."""
    pos = np.asarray(positions, np.float64).reshape(-1)
    if pos.size == 0:
        raise ValueError("site_bins: no positions")
    if not np.isfinite(pos).all() or (np.diff(pos) < 0).any():
        raise ValueError("site_bins: positions must be finite and ascending")
    width = float(width)
    if not width > 0 or not np.isfinite(width):
        raise ValueError("site_bins: width must be positive")
    n_windows = int(np.floor((pos[-1] - pos[0]) / width)) + 1
    bounds = pos[0] + width * np.arange(n_windows + 1, dtype=np.float64)
    edges = np.searchsorted(pos, bounds, side="left")
    edges[0], edges[-1] = 0, pos.size  # (the last bound lies beyond the last site)
    return np.unique(edges).astype(np.int32)


def tail_states(discretization, times) -> np.ndarray:
    """State cuts for ``capi.Context.decode_pair_cdf(..., tail_states=...)`` from times in generations, as
    ``ASMC.decodePairs(..., tail_times=...)`` makes them: the cut of time ``T`` is the number of states ``k < K`` whose
    interval starts below it, ``discretization[k] < float32(T)`` -- the loop of HMM::getStateThreshold, so the decoding
    time gives the IBD scan's state threshold.  ``discretization`` is ``DecodingQuantities.discretization``: K + 1
    values, the K interval starts and the end of the last interval, which is no state's start and is left out.  A time at
    or below ``discretization[0]`` has no state below it and is refused.  Returns int32 cuts in ``[1, K]``.

    A quantile state ``s`` of the result becomes a time as ``expectedTimes[s]`` (the state's expected coalescence time)
    or ``discretization[s + 1]`` (the end of its interval)."""
    disc = np.asarray(discretization, np.float32).reshape(-1)
    if disc.size < 2:
        raise ValueError("tail_states: the discretization holds K + 1 values, K >= 1")
    disc = disc[:-1]
    t = np.asarray(times, np.float32).reshape(-1)
    cuts = (disc[None, :] < t[:, None]).sum(axis=1).astype(np.int32)
    if (cuts == 0).any():
        bad = float(t[np.nonzero(cuts == 0)[0][0]])
        raise ValueError(f"tail_states: tail time {bad}: no interval of the discretization starts below it")
    return cuts


def state_runs(row):
    """The run-length form of one row of ``per_pair_viterbi_states`` or of ``per_pair_sampled_states`` (``ASMC.samplePairs``; or
    of any row of states): ``(starts, ends, states)``,
    three arrays of one entry a run; run ``r`` is sites ``[starts[r], ends[r])``, all in state ``states[r]``, and
    neighbouring runs differ in state.  ``starts[0] = 0`` and ``ends[-1] = len(row)``; an empty row gives three empty
    arrays.  The piecewise-constant TMRCA track of a pair is ``expectedTimes[states]`` over these segments."""
    row = np.asarray(row).reshape(-1)
    if row.size == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64), row.copy()
    cut = np.flatnonzero(row[1:] != row[:-1]) + 1
    starts = np.concatenate([np.zeros(1, np.int64), cut.astype(np.int64)])
    ends = np.concatenate([cut.astype(np.int64), np.full(1, row.size, np.int64)])
    return starts, ends, row[starts]


def site_widths(genetic_positions) -> np.ndarray:
    """Weights for ``ASMC.decodePairs(..., tail_summary_times=..., site_bins=..., site_weights=...)`` that make
    ``per_pair_bin_tail_lengths`` an expected length in centimorgans: the cM site ``t`` stands for, half the distance
    between its neighbours, ``50 * (gen[min(t + 1, S - 1)] - gen[max(t - 1, 0)])`` with ``genetic_positions`` in Morgans
    as ``Data.geneticPositions`` holds them (the first and the last site get half the distance to their one neighbour).
    Computed in float64 and rounded once; returns float32 ``[S]``."""
    gen = np.asarray(genetic_positions, np.float64).reshape(-1)
    if gen.size == 0:
        raise ValueError("site_widths: no positions")
    if not np.isfinite(gen).all():
        raise ValueError("site_widths: positions must be finite")
    t = np.arange(gen.size)
    return (50.0 * (gen[np.minimum(t + 1, gen.size - 1)] - gen[np.maximum(t - 1, 0)])).astype(np.float32)
