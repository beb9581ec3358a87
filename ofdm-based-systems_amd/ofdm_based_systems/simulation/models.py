"""Simulation orchestrator (simulation/models.py:59-818 of the reference).

Same constructor, strategy maps, ``create_from_simulation_settings`` and result
keys.  ``run()`` keeps the reference's setup (channel, prefix length, power
allocation, bit loading -- host precompute on <= 4096 values) and replaces the
data path with the fused GPU engine (:mod:`ofdm_based_systems.engine`):

* every built-in modulator / prefix / constellation (OFDM or SC-OFDM, cyclic, zero or no
  prefix, QAM or PSK, FIXED or CAPACITY_BASED): the two fused kernels (ofdm_tx / ofdm_rx);
* a user-supplied strategy class: the GPU operators composed as in the reference
  (encode -> modulate -> transmit -> demodulate -> decode), calling its own methods.

``rng_mode='reference'`` (default) draws the bits (PCG64 ``Generator.bytes``) and
the AWGN normals (legacy ``np.random.normal``, real part first) exactly as the
reference does, so seeded runs give the reference's integer error counts.
``rng_mode='philox'`` generates both inside the kernels (Monte-Carlo scale).
"""

from __future__ import annotations

import math
import os
import time
from io import BytesIO
from typing import Any, BinaryIO, Dict, List, Optional, Type

import numpy as np
import torch
from numpy.typing import NDArray

from ofdm_based_systems import _backend as B
from ofdm_based_systems.bits_generation.models import AdaptiveBitsGenerator, IGenerator, RandomBitsGenerator
from ofdm_based_systems.channel.models import ChannelModel
from ofdm_based_systems.configuration.enums import (
    AdaptiveModulationMode,
    ConstellationType,
    EqualizationMethod,
    ModulationType,
    NoiseType,
    PowerAllocationType,
    PrefixType,
)
from ofdm_based_systems.configuration.models import SimulationSettings
from ofdm_based_systems.constellation.adaptive import AdaptiveConstellationMapper
from ofdm_based_systems.constellation.models import (
    IConstellationMapper,
    PSKConstellationMapper,
    QAMConstellationMapper,
)
from ofdm_based_systems.engine import LinkEngine
from ofdm_based_systems.equalization.models import MMSEEqualizator, NoEqualizator, ZeroForcingEqualizator
from ofdm_based_systems.modulation.models import IModulator, OFDMModulator, SingleCarrierOFDMModulator
from ofdm_based_systems.noise.models import AWGNoiseModel, NoNoiseModel
from ofdm_based_systems.power_allocation.models import UniformPowerAllocation, WaterfillingPowerAllocation
from ofdm_based_systems.prefix.models import CyclicPrefixScheme, NoPrefixScheme, ZeroPaddingPrefixScheme
from ofdm_based_systems.serial_parallel.models import SerialToParallelConverter

# channel used when no CIR is configured (channel_type FLAT), simulation/models.py:237-245
DEFAULT_CHANNEL = np.array(
    [
        0.7767824138452235072 + 0.4560896742466611919j,
        -0.06669848996328063551 + 0.2839935704583463338j,
        0.1398968327715586490 - 0.1591963958343969865j,
        0.02229949514514480494 + 0.2409945439452868821j,
    ],
    dtype=np.complex128,
)

_EQ_KIND = {EqualizationMethod.NONE: B.EQ_NONE, EqualizationMethod.ZF: B.EQ_ZF,
            EqualizationMethod.MMSE: B.EQ_MMSE}


def read_bits_from_stream(stream: BinaryIO) -> List[int]:
    """All bits of a byte stream, MSB first; rewinds the stream (simulation/models.py:59-69)."""
    data = stream.read()
    stream.seek(0)
    return np.unpackbits(np.frombuffer(data, dtype=np.uint8)).astype(int).tolist()


def _stream_bytes(stream: BinaryIO) -> np.ndarray:
    data = np.frombuffer(stream.read(), dtype=np.uint8).copy()
    stream.seek(0)
    return data


class Simulation:
    CONSTELLATION_SCHEME_MAPPERS = {
        ConstellationType.QAM: QAMConstellationMapper,
        ConstellationType.PSK: PSKConstellationMapper,
    }
    MODULATOR_SCHEME_MAPPERS = {
        ModulationType.OFDM: OFDMModulator,
        ModulationType.SC_OFDM: SingleCarrierOFDMModulator,
    }
    PREFIX_SCHEME_MAPPERS = {
        PrefixType.NONE: NoPrefixScheme,
        PrefixType.CYCLIC: CyclicPrefixScheme,
        PrefixType.ZERO: ZeroPaddingPrefixScheme,
    }
    EQUALIZATOR_SCHEME_MAPPERS = {
        EqualizationMethod.NONE: NoEqualizator,
        EqualizationMethod.ZF: ZeroForcingEqualizator,
        EqualizationMethod.MMSE: MMSEEqualizator,
    }
    NOISE_SCHEME_MAPPERS = {NoiseType.AWGN: AWGNoiseModel, NoiseType.NONE: NoNoiseModel}
    POWER_ALLOCATION_MAPPERS = {
        PowerAllocationType.UNIFORM: UniformPowerAllocation,
        PowerAllocationType.WATERFILLING: WaterfillingPowerAllocation,
    }

    def __init__(
        self,
        num_bits: Optional[int] = None,
        num_symbols: Optional[int] = None,
        num_subcarriers: int = 64,
        constellation_order: int = 16,
        constellation_scheme: ConstellationType = ConstellationType.QAM,
        modulator_type: ModulationType = ModulationType.OFDM,
        prefix_scheme: PrefixType = PrefixType.CYCLIC,
        prefix_length_ratio: float = 1.0,
        equalizator_type: EqualizationMethod = EqualizationMethod.MMSE,
        snr_db: float = 20.0,
        noise_scheme: NoiseType = NoiseType.AWGN,
        power_allocation_type: PowerAllocationType = PowerAllocationType.UNIFORM,
        adaptive_modulation_mode: AdaptiveModulationMode = AdaptiveModulationMode.FIXED,
        min_constellation_order: int = 4,
        max_constellation_order: int = 256,
        desired_symbol_error_rate: float = 1e-3,
        channel_impulse_response: Optional[NDArray[np.complex128]] = None,
        verbose: bool = True,
        *,
        rng_mode: str = "reference",
        seed: Optional[int] = None,
        precision: str = "f64",
        batch_symbols: Optional[int] = None,
        received_symbols_keep: int = 64,
        make_plot: bool = True,
        process_group=None,
        subcarrier_profile: bool = False,
        papr_ccdf: bool = False,
        papr_edges_db=None,
        clip_db: Optional[float] = None,
        frame_symbols: Optional[int] = None,
        constellation_density: Optional[int] = None,
        constellation_density_extent: Optional[float] = None,
        soft_bins: Optional[int] = None,
        soft_extent: Optional[float] = None,
        soft_weights=None,
    ):
        """soft_bins: B: also return the soft decisions of the whole run -- for every compared bit the max-log
        distance difference, in units of the subcarrier's squared minimum distance (times ``soft_weights``:
        None, "csi" or one weight per subcarrier), binned on the GPU into B bins (even, <= 256) over
        [-L, L), L = ``soft_extent`` (default 8), conditioned on the transmitted bit
        (engine.SoftDecisions, ``LinkEngine.run(soft=B)``, ofdm_rx_soft): the key ``soft_decisions`` =
        {``bins``, ``extent``, ``counts`` (nested lists [20][2][B]), ``invalid``, ``num_bits``,
        ``gmi_bits_per_subcarrier``, ``gmi_scale`` (bits per subcarrier -> the LLR scale chosen)}.  Without
        it the result dict is unchanged.  Square QAM only; needs the fused path (the built-in modulators,
        prefixes and constellations); not combined with ``subcarrier_profile``, ``frame_symbols``,
        ``constellation_density`` or ``run_sweep``.

        constellation_density: G: also return where the received points of the whole run fall in the
        I/Q plane -- every equalised point binned on the GPU into a G x G grid (G <= 128) over the square
        [-L, L)^2, L = ``constellation_density_extent`` (default 1.5 times the constellation's largest
        coordinate) (engine.ConstellationDensity, ``LinkEngine.run(density=G)``, ofdm_rx_density): the key
        ``constellation_density`` = {``bins``, ``extent``, ``counts`` (nested lists, row = imaginary
        bin), ``outside``, ``num_points``}.  Without it the result dict is unchanged; ``constellation_plot``
        stays the scatter of the tapped symbols.  Needs the fused path (the built-in modulators, prefixes
        and constellations); not combined with ``subcarrier_profile``, ``frame_symbols`` or ``run_sweep``.

        frame_symbols: F: also return when the errors fall -- the bit errors of every frame of F
        consecutive OFDM symbols, accumulated on the GPU (engine.FrameStats, ``LinkEngine.run(
        frame_symbols=F)``, ofdm_rx_frames): the keys ``frame_symbols``, ``num_frames`` (full frames),
        ``frame_errors``, ``frame_error_rate``, ``ber_std_error`` (None with fewer than two full frames
        or when a trailing partial byte is not compared) and ``bit_errors_per_frame`` (a list, a
        trailing partial frame included).  Without it the result dict is unchanged.  Needs the fused
        path (the built-in modulators, prefixes and constellations); not combined with
        ``subcarrier_profile`` or ``run_sweep``.

        clip_db: limit the envelope of the transmitted samples at ``clip_db`` dB above the nominal
        mean sample power (a soft limiter directly after the IFFT -- for SC-OFDM on the mapped points --
        before the guard and the channel; ``LinkEngine(clip_db=...)``, ofdm_tx_clip).  Every reported
        figure then describes the clipped stream, and the result gains ``clip_db``, ``clipped_samples``
        and ``clipped_fraction``.  Without it the result dict is unchanged.  Needs the fused path and
        constellation orders up to 256; not combined with ``papr_ccdf``.

        papr_ccdf: also return the distribution of the per-symbol PAPR of the transmitted stream,
        binned on the GPU over every OFDM symbol (engine.PaprStats, ``LinkEngine.papr``): the key
        ``papr_ccdf`` = {``edges_db``, ``ccdf``, ``histogram``, ``num_ofdm_symbols``} as lists, at
        ``papr_edges_db`` (default: -0.125 + 0.25 j dB, j < 64).  Without it the result dict is
        unchanged.  Needs the fused path, and constellation orders up to 256.

        subcarrier_profile: also return the run's per-subcarrier results, accumulated on the GPU over
        every OFDM symbol (engine.SubcarrierProfile): the keys ``bit_errors_per_subcarrier``,
        ``symbol_errors_per_subcarrier``, ``error_power_per_subcarrier`` (sum of |z - c|^2 against the
        transmitted point) and ``mer_db_per_subcarrier``.  Without it the result dict is unchanged.
        Needs the fused path (the built-in modulators, prefixes and constellations).  A Simulation
        taps ``received_symbols_keep`` = 64 symbols by default, so it takes the generic profile
        kernel; ``received_symbols_keep=0`` with ``rng_mode='philox'`` reaches the throughput
        receivers' profile kernels on the complex128 bench shapes."""
        if num_bits is None and num_symbols is None:
            raise ValueError("Either num_bits or num_symbols must be provided.")
        if num_bits is not None and num_symbols is not None:
            raise ValueError("Only one of num_bits or num_symbols should be provided.")
        if rng_mode not in ("reference", "philox"):
            raise ValueError("rng_mode must be 'reference' or 'philox'")
        self.num_bits = num_bits
        self.num_symbols = num_symbols
        self.num_subcarriers = num_subcarriers
        self.constellation_order = constellation_order
        self.constellation_scheme = constellation_scheme
        self.modulator_type = modulator_type
        self.prefix_scheme = prefix_scheme
        self.prefix_length_ratio = prefix_length_ratio
        self.equalizator_type = equalizator_type
        self.snr_db = snr_db
        self.noise_scheme = noise_scheme
        self.power_allocation_type = power_allocation_type
        self.adaptive_modulation_mode = adaptive_modulation_mode
        self.min_constellation_order = min_constellation_order
        self.max_constellation_order = max_constellation_order
        self.desired_symbol_error_rate = desired_symbol_error_rate
        self.channel_impulse_response = channel_impulse_response
        self.verbose = verbose
        self.rng_mode = rng_mode
        self.seed = seed
        self.precision = precision
        self.batch_symbols = batch_symbols
        self.received_symbols_keep = received_symbols_keep
        self.make_plot = make_plot
        self.process_group = process_group
        self.subcarrier_profile = subcarrier_profile
        self.papr_ccdf = papr_ccdf
        self.papr_edges_db = papr_edges_db
        self.clip_db = clip_db
        self.frame_symbols = frame_symbols
        self.constellation_density = constellation_density
        self.constellation_density_extent = constellation_density_extent
        self.soft_bins = soft_bins
        self.soft_extent = soft_extent
        self.soft_weights = soft_weights

    def _log(self, message: str) -> None:
        if self.verbose:
            print(message)

    @classmethod
    def create_from_simulation_settings(cls, simulation_settings: SimulationSettings) -> List["Simulation"]:
        """One Simulation per SNR; CUSTOM channels load their .npy relative to the cwd (:167-188)."""
        s = simulation_settings
        cir = None
        if s.channel_type.value == "CUSTOM":
            path = s.channel_model_path
            if not path:
                raise ValueError("channel_model_path must be specified when channel_type is CUSTOM")
            if not path.startswith("/"):
                path = os.path.abspath(path)
            if not os.path.exists(path):
                raise FileNotFoundError(f"Channel model file not found: {path}")
            try:
                cir = np.load(path)  # allow_pickle=False (default)
            except Exception as e:  # noqa: BLE001
                raise ValueError(f"Failed to load channel model from {path}: {e}")
        extra = {"rng_mode": s.rng_mode, "seed": s.seed, "precision": s.precision,
                 "batch_symbols": s.batch_symbols, "clip_db": s.clip_db, "frame_symbols": s.frame_symbols,
                 "constellation_density": s.constellation_density,
                 "constellation_density_extent": s.constellation_density_extent,
                 "soft_bins": s.soft_bins, "soft_extent": s.soft_extent, "soft_weights": s.soft_weights}
        return [
            cls(num_bits=s.num_bits, num_symbols=s.num_symbols, num_subcarriers=s.num_bands,
                constellation_order=s.constellation_order, constellation_scheme=s.constellation_type,
                modulator_type=s.modulation_type, prefix_scheme=s.prefix_type,
                prefix_length_ratio=s.prefix_length_ratio, equalizator_type=s.equalization_method,
                snr_db=snr, noise_scheme=s.noise_type, power_allocation_type=s.power_allocation_type,
                adaptive_modulation_mode=s.adaptive_modulation_mode,
                min_constellation_order=s.min_constellation_order,
                max_constellation_order=s.max_constellation_order,
                desired_symbol_error_rate=s.desired_symbol_error_rate, channel_impulse_response=cir, **extra)
            for snr in s.signal_noise_ratios
        ]

    # ------------------------------------------------------------------ helpers
    def _channel_gains(self, h_raw: np.ndarray) -> np.ndarray:
        """|fft(h_raw, N)|^2 of the un-normalised CIR (simulation/models.py:278-279), on the GPU."""
        plan = B.Plan(n_fft=self.num_subcarriers, h_raw=h_raw)
        H = torch.empty(self.num_subcarriers, dtype=torch.complex128, device=B.device())
        g = torch.empty(self.num_subcarriers, dtype=torch.float64, device=B.device())
        B.check(B.lib().ofdm_plan_response(plan.handle, B.stream_ptr(), B.ptr(H), B.ptr(g)))
        return g.cpu().numpy()

    def _plot(self, received: np.ndarray, mapper: IConstellationMapper, ber: float, papr_db: float,
              title: str, orders: np.ndarray):
        if not self.make_plot:
            return None
        import matplotlib

        matplotlib.use("Agg", force=False)
        import matplotlib.pyplot as plt
        from PIL import Image

        fig = plt.figure(figsize=(8, 8))
        ax = fig.add_subplot(1, 1, 1)
        ax.scatter(received.real, received.imag, color="blue", marker=".", alpha=0.1, label="Received Symbols")
        pts = mapper.constellation
        ax.scatter(pts.real, pts.imag, color="red", marker="o", label="Ideal Constellation Points")
        ax.set_title(title)
        ax.set_xlabel("In-Phase")
        ax.set_ylabel("Quadrature")
        ax.axhline(0, color="black", lw=0.5)
        ax.axvline(0, color="black", lw=0.5)
        ax.legend(loc="upper right")
        ax.grid(True)
        ax.set_xlim(-1.5, 1.5)
        ax.set_ylim(-1.5, 1.5)
        fig.text(0.15, 0.75, f"BER: {ber:.6f}\nSNR: {self.snr_db} dB\nPAPR: {papr_db:.2f} dB", fontsize=10,
                 bbox=dict(facecolor="white", alpha=0.5))
        buf = BytesIO()
        fig.savefig(buf, format="png")
        plt.close(fig)
        buf.seek(0)
        return Image.open(buf)

    # ------------------------------------------------------------------ run
    def run(self) -> Dict[str, Any]:
        return self._run()

    @classmethod
    def run_sweep(cls, simulations: List["Simulation"]) -> List[Dict[str, Any]]:
        """The results of ``[s.run() for s in simulations]`` for the simulations of one SNR sweep
        (the list create_from_simulation_settings returns) from ONE engine sweep
        (LinkEngine.run_sweep): the stream is transmitted once and received at every SNR, where
        running them one by one transmits it again per point.  One result dict per simulation, with
        the keys and values ``run()`` gives (``transmission_time_ms`` is the whole sweep's).

        Raises ValueError unless the simulations differ only in ``snr_db``, use
        ``rng_mode='philox'``, are FIXED mode with the built-in strategies and AWGN, and have
        ``received_symbols_keep == 0`` and no ``subcarrier_profile`` (the sweep receiver has no
        caller streams, no plan per point, no received-symbol tap and no profile), or if they set
        ``frame_symbols`` (:meth:`run_frame_sweep` is the sweep with the frame record)."""
        return cls._sweep("run_sweep", simulations, frames=False)

    @classmethod
    def run_frame_sweep(cls, simulations: List["Simulation"]) -> List[Dict[str, Any]]:
        """:meth:`run_sweep` for simulations with a common ``frame_symbols``: the results of
        ``[s.run() for s in simulations]`` -- the frame keys ``frame_symbols``, ``num_frames``,
        ``frame_errors``, ``frame_error_rate``, ``ber_std_error`` and ``bit_errors_per_frame`` among them
        -- from ONE engine frame sweep (LinkEngine.run_frame_sweep): a frame-error-rate curve from one
        transmit.  ``transmission_time_ms`` is the whole sweep's.

        Raises ValueError for what :meth:`run_sweep` refuses, except that ``frame_symbols`` must be set;
        ``constellation_density``, ``subcarrier_profile`` and a received-symbol tap are still refused."""
        return cls._sweep("run_frame_sweep", simulations, frames=True)

    @classmethod
    def _sweep(cls, who: str, simulations, frames: bool) -> List[Dict[str, Any]]:
        """run_sweep (``frames`` False) and run_frame_sweep: the checks, and one engine sweep feeding
        every simulation's _run."""
        sims = list(simulations)
        if not sims:
            return []

        def same(a, b):
            if isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
                return a is not None and b is not None and np.array_equal(a, b)
            return a is b or a == b

        first = vars(sims[0])
        for s in sims[1:]:
            for key, val in vars(s).items():
                if key != "snr_db" and not same(val, first[key]):
                    raise ValueError(f"{who}: the simulations differ in more than snr_db ({key})")
        s0 = sims[0]
        if s0.rng_mode != "philox":
            raise ValueError(f"{who} needs rng_mode='philox' (the sweep receiver generates its streams)")
        builtin = (s0._builtin_strategies()
                   and cls.NOISE_SCHEME_MAPPERS.get(s0.noise_scheme, AWGNoiseModel) is AWGNoiseModel)
        if s0.adaptive_modulation_mode != AdaptiveModulationMode.FIXED or not builtin:
            raise ValueError(f"{who} needs FIXED mode with the built-in modulators, prefixes, constellations "
                             "and AWGN (adaptive loading is a different plan per SNR)")
        if s0.received_symbols_keep != 0 or s0.subcarrier_profile:
            raise ValueError(f"{who} needs received_symbols_keep=0 and no subcarrier_profile")
        if s0.frame_symbols is not None and not frames:
            raise ValueError("run_sweep with frame_symbols: run_sweep keeps no frame record; the sweep with the "
                             "record of every point is run_frame_sweep")
        if s0.frame_symbols is None and frames:
            raise ValueError("run_frame_sweep needs frame_symbols set on the simulations (without it: run_sweep)")

        if s0.constellation_density is not None:
            raise ValueError(f"{who} with constellation_density: the sweep receiver keeps no density record; "
                             "run the simulations one by one")

        if s0.soft_bins is not None:
            raise ValueError(f"{who} with soft_bins: the sweep receiver keeps no soft record; "
                             "run the simulations one by one")

        swept: List[Any] = []  # the engine sweep's LinkStats, filled by the first simulation

        def link(k):
            def stats(make_engine, n_sym, seed, valid_bits):
                if not swept:
                    kw = dict(seed=seed, group=s0.process_group, batch=s0.batch_symbols, n_valid_bits=valid_bits)
                    snrs = [s.snr_db for s in sims]
                    eng = make_engine()
                    swept.extend(eng.run_frame_sweep(n_sym, snrs, s0.frame_symbols, **kw) if frames
                                 else eng.run_sweep(n_sym, snrs, **kw))
                return swept[k]
            return stats

        return [s._run(link(k)) for k, s in enumerate(sims)]

    def _check_clip(self, orders=None) -> None:
        """What a clip level is not combined with, refused before the run: the PAPR histogram (it bins
        the unclipped stream), user-supplied strategy classes (the composed path has no limiter) and
        orders above 256 (``orders``: the adaptive loading's, once known)."""
        if self.papr_ccdf:
            raise ValueError("papr_ccdf with clip_db: the PAPR histogram of a clipped stream is not built")
        if not self._builtin_strategies():
            raise ValueError("clip_db needs the built-in modulators, prefixes and constellations")
        top = (self.constellation_order if self.adaptive_modulation_mode == AdaptiveModulationMode.FIXED
               else 0 if orders is None else int(np.max(orders, initial=0)))
        if top > 256:
            raise ValueError(f"clip_db takes constellation orders up to 256, got {top}")

    def _builtin_strategies(self) -> bool:
        """Whether the modulator, prefix and constellation are the built-in classes (the fused path's)."""
        return (self.MODULATOR_SCHEME_MAPPERS.get(self.modulator_type, OFDMModulator) in (
                    OFDMModulator, SingleCarrierOFDMModulator)
                and self.PREFIX_SCHEME_MAPPERS.get(self.prefix_scheme, NoPrefixScheme) in (
                    CyclicPrefixScheme, ZeroPaddingPrefixScheme, NoPrefixScheme)
                and self.CONSTELLATION_SCHEME_MAPPERS.get(self.constellation_scheme, QAMConstellationMapper) in (
                    QAMConstellationMapper, PSKConstellationMapper))

    def _check_frames(self) -> None:
        """What a frame record is not combined with, refused before the run: user-supplied strategy
        classes (the composed path keeps no record), the per-subcarrier profile, a bad frame length."""
        F = self.frame_symbols
        if isinstance(F, bool) or not isinstance(F, (int, np.integer)) or F < 1:
            raise ValueError(f"frame_symbols = {F!r} is not a positive number of OFDM symbols")
        if not self._builtin_strategies():
            raise ValueError("frame_symbols needs the built-in modulators, prefixes and constellations")
        if self.subcarrier_profile:
            raise ValueError("frame_symbols with subcarrier_profile: the receiver with both records is not built")

    def _check_density(self) -> None:
        """What a density record is not combined with, refused before the run: user-supplied strategy
        classes (the composed path keeps no record), the per-subcarrier profile, the frame record, a bad
        grid."""
        from ofdm_based_systems.engine import density_grid

        L = self.constellation_density_extent
        density_grid(self.constellation_density, 1.0 if L is None else L)  # (ValueError for a bad G or L)
        if not self._builtin_strategies():
            raise ValueError("constellation_density needs the built-in modulators, prefixes and constellations")
        if self.subcarrier_profile:
            raise ValueError("constellation_density with subcarrier_profile: the receiver with both records is "
                             "not built")
        if self.frame_symbols is not None:
            raise ValueError("constellation_density with frame_symbols: the receiver with both records is not built")

    def _check_soft(self) -> None:
        """What a soft record is not combined with, refused before the run: user-supplied strategy classes
        (the composed path keeps no record), the other records, a bad B or L."""
        from ofdm_based_systems.engine import soft_grid

        soft_grid(self.soft_bins, 8.0 if self.soft_extent is None else self.soft_extent)  # (ValueError)
        if not self._builtin_strategies():
            raise ValueError("soft_bins needs the built-in modulators, prefixes and constellations")
        for other, name in ((self.subcarrier_profile, "subcarrier_profile"), (self.frame_symbols is not None, "frame_symbols"),
                            (self.constellation_density is not None, "constellation_density")):
            if other:
                raise ValueError(f"soft_bins with {name}: the receiver with both records is not built")

    def _run(self, link=None) -> Dict[str, Any]:
        """run(); ``link`` (run_sweep): a callable (make_engine, n_sym, seed, valid_bits) -> LinkStats
        standing in for this simulation's own engine run."""
        results: Dict[str, Any] = {}
        if self.clip_db is not None:
            self._check_clip()  # (before anything is launched)
        if self.frame_symbols is not None:
            self._check_frames()
        if self.constellation_density is not None:
            self._check_density()
        if self.soft_bins is not None:
            self._check_soft()
        elif self.soft_extent is not None or self.soft_weights is not None:
            raise ValueError("soft_extent / soft_weights without soft_bins")
        sp = SerialToParallelConverter()
        noise_model = self.NOISE_SCHEME_MAPPERS.get(self.noise_scheme, AWGNoiseModel)()
        h_raw = np.asarray(DEFAULT_CHANNEL if self.channel_impulse_response is None
                           else self.channel_impulse_response, dtype=np.complex128)
        channel = ChannelModel(impulse_response=h_raw, snr_db=self.snr_db, noise_model=noise_model)
        cp = 0 if self.prefix_scheme == PrefixType.NONE else int(self.prefix_length_ratio * channel.order)
        prefix_scheme = self.PREFIX_SCHEME_MAPPERS.get(self.prefix_scheme, NoPrefixScheme)(prefix_length=cp)
        N = self.num_subcarriers
        gains = self._channel_gains(h_raw)
        noise_power = 10 ** (-self.snr_db / 10)
        water_level: Optional[float] = None
        base_mapper: Type[IConstellationMapper] = self.CONSTELLATION_SCHEME_MAPPERS.get(
            self.constellation_scheme, QAMConstellationMapper)

        if self.adaptive_modulation_mode == AdaptiveModulationMode.CAPACITY_BASED:
            # bit loading from the allocation with P_tot = N (simulation/models.py:289-395)
            if self.power_allocation_type == PowerAllocationType.WATERFILLING:
                allocation = WaterfillingPowerAllocation(N, gains, noise_power).allocate()
                level = allocation + noise_power / gains
                water_level = float(np.mean(level[allocation > 1e-10]))
            else:
                allocation = UniformPowerAllocation(N, N).allocate()
            orders = np.array([base_mapper.calculate_bit_loading_order(
                ser=self.desired_symbol_error_rate, snr=p * g / noise_power) for p, g in zip(allocation, gains)],
                dtype=np.int64)
            if self.clip_db is not None:
                self._check_clip(orders)
            mapper: IConstellationMapper = AdaptiveConstellationMapper(orders, base_mapper, N)
            bps = int(np.sum(mapper.get_bits_per_subcarrier()))
            if self.num_symbols is not None:
                n_ofdm = self.num_symbols
            else:
                if bps == 0:
                    raise ValueError("All subcarriers have zero order - cannot transmit data")
                n_ofdm = self.num_bits // bps
            bits_gen: IGenerator = AdaptiveBitsGenerator(mapper.get_bits_per_subcarrier(), n_ofdm)
            total_bits = bits_gen.get_total_bits()
        else:
            orders = np.full(N, self.constellation_order, dtype=np.int64)
            mapper = base_mapper(order=self.constellation_order)
            bits_gen = RandomBitsGenerator()
            total_bits = self.num_bits
            if self.num_symbols is not None:
                total_bits = self.num_symbols * int(np.log2(self.constellation_order))
            allocation = None

        results.update({
            "num_bits": self.num_bits,
            "num_symbols": self.num_symbols,
            "num_subcarriers": N,
            "constellation_order": self.constellation_order,
            "constellation_scheme": self.constellation_scheme.name,
            "modulator_type": self.modulator_type.name,
            "prefix_scheme": self.prefix_scheme.name,
            "prefix_acronym": prefix_scheme.acronym,
            "equalizator_type": self.equalizator_type.name,
            "snr_db": self.snr_db,
            "noise_scheme": self.noise_scheme.name,
            "power_allocation_type": self.power_allocation_type.name,
            "power_allocation_acronym": (
                "WF" if self.power_allocation_type == PowerAllocationType.WATERFILLING else "UNIFORM"),
            "adaptive_modulation_mode": self.adaptive_modulation_mode.name,
            "constellation_order_per_subcarrier": orders.tolist(),
            "water_level": water_level,
            "title": f"{prefix_scheme.acronym}-{self.modulator_type.name}-{self.equalizator_type.name}",
            "subtitle": (f"{self.constellation_order}{self.constellation_scheme.name}-"
                         f"SNR{self.snr_db}dB-{self.power_allocation_type.name}"),
        })
        if total_bits is None:
            raise ValueError("Total bits could not be determined.")

        adaptive = self.adaptive_modulation_mode == AdaptiveModulationMode.CAPACITY_BASED
        if adaptive:
            n_ofdm_syms = n_ofdm
            valid_bits = (total_bits // 8) * 8
            # AdaptiveConstellationMapper.encode needs whole OFDM symbols, both for the tx stream
            # and for the re-encode of the received (whole-byte) stream (simulation/models.py:604)
            for nbits in (8 * math.ceil(total_bits / 8), valid_bits):
                if nbits % bps:
                    raise ValueError(f"Bits length ({nbits}) must be multiple of bits_per_symbol ({bps})")
        else:
            b = int(np.log2(self.constellation_order))
            n_const = math.ceil(8 * math.ceil(total_bits / 8) / b)
            if n_const % N:
                raise ValueError("Length of data must be divisible by number of streams.")
            n_ofdm_syms = n_const // N
            valid_bits = 8 * math.ceil(total_bits / 8)

        # FIXED-mode allocation: computed, reported, never applied (simulation/models.py:483-509)
        if not adaptive:
            if self.power_allocation_type == PowerAllocationType.WATERFILLING:
                allocation = WaterfillingPowerAllocation(1.0, gains, noise_power).allocate()
                level = allocation + noise_power / gains
                water_level = float(np.mean(level[allocation > 1e-10]))
            else:
                allocation = UniformPowerAllocation(1.0, N).allocate()
        results["allocated_power"] = allocation.tolist()

        # ---------------- data path
        reference = self.rng_mode == "reference"
        tx_bytes = _stream_bytes(bits_gen.generate_bits(total_bits)) if reference else None
        # every built-in strategy runs on the fused kernels (SC-OFDM, zero padding and PSK on
        # the generic kernel); a user-supplied strategy class falls back to the composed
        # GPU operators, which call its own methods
        mod_cls = self.MODULATOR_SCHEME_MAPPERS.get(self.modulator_type, OFDMModulator)
        pre_cls = self.PREFIX_SCHEME_MAPPERS.get(self.prefix_scheme, NoPrefixScheme)
        fused = (mod_cls in (OFDMModulator, SingleCarrierOFDMModulator)
                 and pre_cls in (CyclicPrefixScheme, ZeroPaddingPrefixScheme, NoPrefixScheme)
                 and type(mapper) in (QAMConstellationMapper, PSKConstellationMapper, AdaptiveConstellationMapper)
                 and not (adaptive and self.modulator_type == ModulationType.SC_OFDM)
                 and len(h_raw) - 1 <= N and cp <= N)
        if not fused and not reference:
            raise ValueError("rng_mode='philox' needs the built-in modulators, prefixes and constellations")
        if not fused and self.subcarrier_profile:
            raise ValueError("subcarrier_profile needs the built-in modulators, prefixes and constellations")
        if not fused and self.frame_symbols is not None:  # (_check_frames saw the strategy classes)
            raise ValueError("frame_symbols needs the fused path (channel order and prefix within n_fft)")
        if not fused and self.constellation_density is not None:  # (_check_density saw the strategy classes)
            raise ValueError("constellation_density needs the fused path (channel order and prefix within n_fft)")
        if not fused and self.soft_bins is not None:  # (_check_soft saw the strategy classes)
            raise ValueError("soft_bins needs the fused path (channel order and prefix within n_fft)")
        if not fused and self.papr_ccdf:
            raise ValueError("papr_ccdf needs the built-in modulators, prefixes and constellations")
        if not fused and self.clip_db is not None:
            raise ValueError("clip_db needs the fused path (the built-in strategies, channel order and prefix "
                             "within n_fft)")
        if not fused and link is not None:
            raise ValueError("run_sweep needs the fused path (channel order and prefix within n_fft)")
        t0 = time.perf_counter()
        if fused:
            luts, sc = (mapper.lut_tables() if adaptive else ([mapper.constellation], None))
            prec = B.OFDM_F32 if self.precision == "f32" else B.OFDM_F64
            def make_engine():
                return LinkEngine(N, cp, h_raw, _EQ_KIND[self.equalizator_type], luts, sc, prec,
                                  prefix=B.PREFIX_ZERO if pre_cls is ZeroPaddingPrefixScheme else B.PREFIX_CYCLIC,
                                  modulator=B.MOD_SC if mod_cls is SingleCarrierOFDMModulator else B.MOD_OFDM,
                                  **({} if self.clip_db is None else {"clip_db": self.clip_db}))

            noise_on = isinstance(noise_model, AWGNoiseModel)
            normals = None
            if reference and noise_on:
                n_samp = n_ofdm_syms * (N + cp)
                normals = (np.random.normal(size=n_samp), np.random.normal(size=n_samp))
            seed = self.seed if self.seed is not None else 0
            if link is not None:
                st = link(make_engine, n_ofdm_syms, seed, valid_bits)
            else:
                eng = make_engine()
                st = eng.run(n_ofdm_syms, self.snr_db, bits=tx_bytes, normals=normals, seed=seed,
                             noise_on=noise_on, keep_symbols=self.received_symbols_keep,
                             group=self.process_group, batch=self.batch_symbols,
                             n_valid_bits=valid_bits, profile=self.subcarrier_profile,
                             **({} if self.frame_symbols is None else {"frame_symbols": self.frame_symbols}),
                             **({} if self.constellation_density is None else {
                                 "density": self.constellation_density,
                                 "density_extent": self.constellation_density_extent}),
                             **({} if self.soft_bins is None else {
                                 "soft": self.soft_bins, "soft_extent": self.soft_extent,
                                 "soft_weights": self.soft_weights}))
            if self.papr_ccdf:
                # the per-symbol PAPR distribution of the stream just transmitted: the same plan, seed
                # and (reference mode) the run's own bits
                papr = (eng if link is None else make_engine()).papr(
                    n_ofdm_syms, seed=seed, bits=tx_bytes, edges_db=self.papr_edges_db,
                    group=self.process_group, batch=self.batch_symbols)
            torch.cuda.synchronize()
            bit_errors, symbol_errors, papr_db = st.bit_errors, st.symbol_errors, st.papr_db
            received = st.received if st.received is not None else np.zeros(0, np.complex128)
            n_syms_total = n_ofdm_syms * N
            profile = st.profile
        else:
            bit_errors, symbol_errors, papr_db, received, n_syms_total = self._composed_path(
                tx_bytes, mapper, prefix_scheme, channel, sp, valid_bits)
        elapsed = time.perf_counter() - t0

        ber = bit_errors / total_bits if total_bits > 0 else 0.0
        ser = symbol_errors / n_syms_total if n_syms_total > 0 else 0.0
        results.update({
            "papr_db": papr_db,
            "bit_errors": bit_errors,
            "symbol_errors": symbol_errors,
            "total_bits": total_bits,
            "bit_error_rate": ber,
            "symbol_error_rate": ser,
            "received_symbols": received,
        })
        if self.subcarrier_profile:
            results.update({
                "bit_errors_per_subcarrier": profile.bit_errors,
                "symbol_errors_per_subcarrier": profile.symbol_errors,
                "error_power_per_subcarrier": profile.error_power,
                "mer_db_per_subcarrier": profile.mer_db,
            })
        if self.frame_symbols is not None:
            fr = st.frames
            results.update({
                "frame_symbols": fr.frame_symbols,
                "num_frames": fr.n_full,
                "frame_errors": fr.frame_errors,
                "frame_error_rate": fr.fer,
                "ber_std_error": fr.ber_stderr,
                "bit_errors_per_frame": fr.bit_errors.tolist(),
            })
        if self.constellation_density is not None:
            d = st.density
            results["constellation_density"] = {
                "bins": d.bins,
                "extent": d.extent,
                "counts": d.counts.tolist(),
                "outside": d.outside,
                "num_points": d.n_points,
            }
        if self.soft_bins is not None:
            sd = st.soft
            results["soft_decisions"] = {
                "bins": sd.bins,
                "extent": sd.extent,
                "counts": sd.counts.tolist(),
                "invalid": sd.invalid,
                "num_bits": sd.n_bits,
                "gmi_bits_per_subcarrier": sd.gmi(),
                "gmi_scale": {str(b): sd.gmi_scale(b) for b in sd.orders},
            }
        if self.clip_db is not None:
            results.update({
                "clip_db": float(self.clip_db),
                "clipped_samples": st.clipped_samples,
                "clipped_fraction": st.clipped_samples / st.clip_samples if st.clip_samples else 0.0,
            })
        if self.papr_ccdf:
            results["papr_ccdf"] = {
                "edges_db": papr.edges_db.tolist(),
                "ccdf": papr.ccdf.tolist(),
                "histogram": papr.histogram.tolist(),
                "num_ofdm_symbols": papr.num_ofdm_symbols,
            }
        results["constellation_plot"] = self._plot(received, mapper, ber, papr_db, results["title"], orders)
        results["transmission_time_ms"] = elapsed * 1000
        results["bitrate_mbps"] = total_bits / 1e6  # the reference reports Mbit, not a rate (:807)
        self._log(f"BER {ber:.6e}  SER {ser:.6e}  PAPR {papr_db:.2f} dB  ({elapsed * 1e3:.1f} ms)")
        return results

    # ------------------------------------------------------------------ composed GPU operators
    def _composed_path(self, tx_bytes, mapper, prefix_scheme, channel, sp, valid_bits):
        """SC-OFDM / zero padding / PSK: the reference's operator chain on GPU operators."""
        N = self.num_subcarriers
        eq = self.EQUALIZATOR_SCHEME_MAPPERS.get(self.equalizator_type, NoEqualizator)(
            channel_frequency_response=self._raw_response(channel), snr_db=self.snr_db)
        modulator: IModulator = self.MODULATOR_SCHEME_MAPPERS.get(self.modulator_type, OFDMModulator)(
            num_subcarriers=N, prefix_scheme=prefix_scheme, equalizator=eq)
        symbols = mapper.encode(BytesIO(tx_bytes.tobytes()))
        x = modulator.modulate(sp.to_parallel(symbols, N))
        p = np.abs(x) ** 2
        papr_db = float(10 * np.log10(np.max(p) / np.mean(p))) if np.mean(p) > 0 else float("inf")
        y = channel.transmit(sp.to_serial(x))
        Z = modulator.demodulate(sp.to_parallel(y, N + prefix_scheme.prefix_length))
        z = sp.to_serial(Z)
        rx = np.frombuffer(mapper.decode(z).read(), dtype=np.uint8)
        be, se = _compare_on_device(tx_bytes, rx, symbols, mapper, valid_bits)
        keep = z[: self.received_symbols_keep * N]
        return be, se, papr_db, keep, len(symbols)

    def _raw_response(self, channel: ChannelModel) -> np.ndarray:
        """fft(h_raw, N) of the configured (un-normalised) CIR, as the reference's equaliser gets it."""
        plan = B.Plan(n_fft=self.num_subcarriers, h_raw=channel._h_raw)
        H = torch.empty(self.num_subcarriers, dtype=torch.complex128, device=B.device())
        B.check(B.lib().ofdm_plan_response(plan.handle, B.stream_ptr(), B.ptr(H), None))
        return H.cpu().numpy()


def _compare_on_device(tx: np.ndarray, rx: np.ndarray, symbols: np.ndarray, mapper, valid_bits: int):
    """bit_errors = popcount(tx ^ rx) over the compared bits; symbol_errors = symbols != encode(rx)
    (simulation/models.py:596-606)."""
    n = min(len(tx), len(rx))
    a = torch.from_numpy(tx[:n].copy()).to(B.device())
    b = torch.from_numpy(rx[:n].copy()).to(B.device())
    xor = torch.bitwise_xor(a, b)
    tail = min(valid_bits, 8 * n)
    bits = torch.bitwise_and(xor.unsqueeze(1) >> torch.arange(7, -1, -1, device=a.device), 1).reshape(-1)
    be = int(bits[:tail].sum().item())
    recoded = mapper.encode(BytesIO(rx.tobytes()))
    m = min(len(recoded), len(symbols))
    se = int(np.count_nonzero(symbols[:m] != recoded[:m]))
    return be, se
