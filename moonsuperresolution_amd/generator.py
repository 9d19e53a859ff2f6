"""``Generator`` — the drop-in for the reference's ``model`` callable.

The reference's only coupling between its inference driver and its networks is
``pred_dems = self.model(np.array(batch), training=False)`` (process_full_tiles.py:338) followed by
``np.array(pred_dems)[:, :, :, -1] + 0.5`` (:340), where ``model`` is ``GauGAN(image_size, batch_size,
latent_dim)`` / ``CNNSpade(...)`` (process_full_tiles.py:28,48) or ``Pix2Pix().generator``.  This class keeps
that signature — ``Generator(image_size, batch_size, ...)(batch[B,S,S,2], training=False) ->
np.ndarray[B,S,S,1]`` — and runs the hand-written gfx950 kernels of libmoonsr_hip.so underneath.

PyTorch is used for device memory and streams only; all arithmetic happens inside the HIP library.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Mapping, Optional, Union

import numpy as np
import torch

from . import _lib
from .weights import VARIANTS, make_latent_noise, make_weights, weight_shapes


def parse_conv_forms(text: str) -> list:
    """The text of msr_debug_conv_forms -> one dict per line; values that read as integers become ints."""
    ops = []
    for line in text.splitlines():
        d = dict(word.split("=", 1) for word in line.split())
        ops.append({k: int(v) if v.lstrip("-").isdigit() else v for k, v in d.items()})
    return ops


def form_table(image_size: int, batch_size: int, variant: str = "gaugan", flags: int = 0, latent_dim: int = 256) -> dict:
    """msr_debug_form_table, which needs no GPU: {layer: parse_conv_forms dict of its line} of the form table a handle of this
    configuration gets under this process's environment switches, plus "head_fused": 0 | 1.  ValueError for a configuration
    msr_create rejects."""
    lib = _lib.load()
    cfg = _lib.MsrConfig(image_size, batch_size, latent_dim, _lib.VARIANT_IDS[variant], 0, flags)
    buf = C.create_string_buffer(1 << 14)
    _lib.raise_for(lib, None, lib.msr_debug_form_table(C.byref(cfg), buf, len(buf)), "msr_debug_form_table")
    lines = buf.value.decode().splitlines()
    table = {ln.split()[0]: parse_conv_forms(ln.split(None, 1)[1])[0] for ln in lines[:-1]}
    table["head_fused"] = int(lines[-1].split("=")[1])
    return table


F16_MAX = 65504.0

# msr_debug_fill_workspace `what`: the un-zeroed ws.* buffers and the scratch buffers; the interior of the zero-bordered
# buffers (the slots their producers write); their borders
FILL_WORKSPACE, FILL_INTERIOR, FILL_BORDER = 1, 2, 4


class RangeReport:
    """Result of an activation-range scan (msr_range_scan): ``records`` — one dict per narrow activation tensor of the plan, in
    plan order (tensor, format, producer, max_abs, n_total, n_cross_clipped, n_clamped, n_nonfinite); ``embed_bounds`` — one dict
    per conv_gb_resident op, whose embedding cannot be scanned (max_abs holds the host-side bound); ``layers`` — producer index
    -> the producing layer's weight name, for the text.

    ``regime`` follows tests/test_gpu_conv_kernel.py::test_f16c_saturation_regimes: "clamped" if any tensor holds a clamped or
    non-finite element or an embed bound exceeds 65504 (finite and wrong), else "degraded" if any e4m3 cross piece is clipped
    (the conv drops to one fp16 product), else "parity".  An empty report (fp32, bf16x3: no narrow tensor) is "parity"."""

    def __init__(self, records=(), embed_bounds=(), layers=None):
        self.records = [dict(r) for r in records]
        self.embed_bounds = [dict(r) for r in embed_bounds]
        self.layers = dict(layers or {})
        self.note = ""          # what precision="auto" did with an option of the mode it left (appended to the text)

    @property
    def regime(self) -> str:
        if any(r["n_clamped"] + r["n_nonfinite"] > 0 for r in self.records) or \
                any(not (e["max_abs"] <= F16_MAX) for e in self.embed_bounds):
            return "clamped"
        if any(r["n_cross_clipped"] > 0 for r in self.records):
            return "degraded"
        return "parity"

    @property
    def worst(self) -> Optional[dict]:
        """The record that decides the regime: most clamped + non-finite elements, then most clipped cross pieces, then the
        largest max_abs; the first in plan order among equals.  None for an empty report."""
        if not self.records:
            return None
        key = lambda r: (r["n_clamped"] + r["n_nonfinite"], r["n_cross_clipped"], float(r["max_abs"]))   # noqa: E731
        best = self.records[0]
        for r in self.records[1:]:
            if key(r) > key(best):
                best = r
        return best

    def flagged(self) -> list:
        """Names of the tensors with any clipped, clamped or non-finite element, in plan order."""
        return [r["tensor"] for r in self.records if r["n_cross_clipped"] + r["n_clamped"] + r["n_nonfinite"] > 0]

    def __str__(self) -> str:
        w = self.worst
        if w is None:
            return "activation range: parity (no narrow activation tensor in this plan)" + (f"; {self.note}" if self.note else "")
        layer = self.layers.get(w["producer"], "?")
        text = (f"activation range: {self.regime}; worst tensor {w['tensor']} (format {w['format']}, written by op "
                f"{w['producer']}, {layer}): max |a| = {float(w['max_abs']):.6g}, {w['n_cross_clipped']} cross-clipped (|a| > 464), "
                f"{w['n_clamped']} clamped, {w['n_nonfinite']} non-finite of {w['n_total']} elements; "
                f"{len(self.flagged())} of {len(self.records)} tensors flagged")
        over = [e for e in self.embed_bounds if not (e["max_abs"] <= F16_MAX)]
        if over:
            text += f"; embedding bound of {over[0]['tensor']} is {float(over[0]['max_abs']):.6g} > 65504"
        if self.note:
            text += f"; {self.note}"
        return text

    __repr__ = __str__


class Generator:
    """MI355X generator(call).

    Args mirror ``GauGAN(image_size, batch_size, latent_dim=256)`` (spade/models/model.py:341-346):
        image_size, batch_size, latent_dim: as the reference; ``batch_size`` is baked in, like the
            reference's sampler (spade/models/sampling.py:13-15).
        variant: "gaugan" (sampler), "gaugan_no_kl" / "cnn" (mean + variance), "pix2pix".
        weights: name -> float32 array in the reference layouts (see ``weights.weight_shapes``), or an int
            seed for the Keras-default random init (no trained weights ship with the reference).
        eps: the sampler's N(0,1) draw ``[batch_size, latent_dim]`` for "gaugan"; ``None`` draws a fresh one
            per call like ``tf.random.normal`` (sampling.py:13), an int seeds a fixed one (repeatable runs).
        device: HIP device ordinal (one process per GPU).
        precision: conv arithmetic — "f16c" (default: fp16 main term + fp8 cross terms in the convs that fill the chip,
            3-term split-bf16 elsewhere; fp32 accumulation; 3.6-4.7e-5 relative L-inf end to end against the oracle on
            the BASELINE shapes), "bf16x3" (3-term split-bf16 products on the bf16 MFMA everywhere; 1.7-2.0e-5, 13 %
            slower) or "fp32" (exact fp32 MFMA, 3-5e-6, 4x slower).  All three are >= 20x inside the 1e-3 parity bar.  "bf16x3_gbf16" is the
            opt-in faster mode: bf16x3, with 2-term fp16 products (weight rounded to one fp16) in the SPADE
            gamma|beta convs — 2-5e-4 end to end, inside the bar with a small margin.  "fp8" is the declared
            NON-parity mode of BASELINE configs[4] (fp8 e4m3 weights x bf8 e5m2 activations on the block-scaled
            fp8 MFMA in the chip-filling convs): it does not meet the 1e-3 bar.  "f16" is the declared-tolerance fast
            mode of round 3: the f16c data path with the cross terms left out of the two big kernels (one fp16 product
            per element; error stated in tests/test_gpu_baseline_configs.py).  Inputs, outputs, weights and
            every non-conv op (moments, normalisation, epilogues, dense, head) are fp32 in every mode.
            "auto" builds "f16c", runs one call on ``calibrate`` and scans the activation ranges (``range_report``); it keeps
            f16c when the regime is "parity" and rebuilds as "bf16x3" from the same weights otherwise.  ``.precision`` then
            reads the mode chosen and ``.range`` the report that decided it; ``clone()`` clones the chosen mode.
        cross: format of the f16c mode's cross terms in the main convs — "fp8" (default) or "fp6" (opt-in: e2m3 pieces with a
            block scale per pixel and 32 channels, 1.5 instead of 2 MFMA-equivalents per product in the convs that run the
            stream kernel, same parity grade; the measured A/B is in DESIGN.md).  "fp6" goes with precision="f16c", or with
            "auto", which keeps it when it stays on f16c and drops it (``.cross`` reads "fp8", ``.range`` says so) when it
            falls back to bf16x3.
        head: "separate" (default) or "fused" (opt-in, MSR_FLAG_FUSED_HEAD): the last residual conv emits the head's partial
            sums (32 floats per pixel) instead of its 128-channel output and a gather kernel finishes the head.  It goes with
            precision="f16c" and cross="fp8", or with "auto", which keeps it on f16c and drops it with a note in ``.range`` on
            bf16x3.  The plan takes it where that conv runs the stream kernel on whole tiles (``head_fused``); at smaller
            shapes the separate head runs.  Activations beyond fp16's 65504 saturate in the fused head (include/moonsr.h).
        sampler: where the "gaugan" sampler's noise comes from when ``eps`` is None — "torch" (default: ``torch.randn`` once per
            call, as ``tf.random.normal``: it follows torch's global generator and the order of the calls) or "counter" (opt-in:
            msr_sampler_noise fills a persistent [batch_size, latent_dim] device buffer before every call; row b's noise is a
            pure function of ``seed`` and the row's id — ``forward_device(noise_ids=...)``, or (calls * batch_size + b, 0, 0)
            from this instance's call counter, ``reset_sampler``).  Reproducible, independent of how calls are spread over
            ranks, row windows and pipeline handles when the caller's ids are (the tiler's are), and the noise pointer never
            changes, so ``use_graph`` replays.  "counter" goes with variant="gaugan" and eps=None.
        seed: the 64-bit seed of sampler="counter".
        calibrate: the batch [batch_size, S, S, 2] "auto" calibrates on; None = ``synthetic_patches(batch_size, S, seed=0)``.
            Calibration holds for the data it saw: ``DEMSuperResolution(range_check=...)`` checks real tiles.
    """

    def __init__(self, image_size: int, batch_size: int, latent_dim: int = 256, variant: str = "gaugan",
                 weights: Union[int, Mapping[str, np.ndarray]] = 1234, eps: Union[None, int, np.ndarray] = None,
                 device: int = 0, precision: str = "f16c", calibrate=None, cross: str = "fp8", head: str = "separate",
                 sampler: str = "torch", seed: int = 0):
        if variant not in VARIANTS:
            raise ValueError(f"unknown variant {variant!r}; expected one of {VARIANTS}")
        if sampler not in ("torch", "counter"):
            raise ValueError(f"unknown sampler {sampler!r}; expected 'torch' or 'counter'")
        if sampler == "counter" and variant != "gaugan":
            raise ValueError(f"sampler='counter' is the noise of variant='gaugan'; variant {variant!r} draws none")
        if sampler == "counter" and eps is not None:
            raise ValueError("sampler='counter' generates the noise of every call; it does not go with a fixed eps")
        if not 0 <= int(seed) < 1 << 64:
            raise ValueError(f"seed must be in [0, 2^64), got {seed}")
        if cross not in _lib.CROSS_FLAGS:
            raise ValueError(f"unknown cross {cross!r}; expected one of {tuple(_lib.CROSS_FLAGS)}")
        if cross != "fp8" and precision not in ("f16c", "auto"):
            raise ValueError(f"cross={cross!r} is an option of precision='f16c' (or 'auto'), not of {precision!r}")
        if head not in _lib.HEAD_FLAGS:
            raise ValueError(f"unknown head {head!r}; expected one of {tuple(_lib.HEAD_FLAGS)}")
        if head != "separate" and (precision not in ("f16c", "auto") or cross != "fp8" or variant == "pix2pix"):
            raise ValueError(f"head={head!r} is an option of precision='f16c' (or 'auto') with cross='fp8' on the SPADE variants, "
                             f"not of precision={precision!r}, cross={cross!r}, variant={variant!r}")
        if precision == "auto":
            # resolved here, above the flag table: try the fast default, keep it only in the parity regime
            if isinstance(weights, (int, np.integer)):
                weights = make_weights(variant, image_size, latent_dim, seed=int(weights))
            self.__init__(image_size, batch_size, latent_dim, variant, weights, eps, device, "f16c", cross=cross, head=head,
                          sampler=sampler, seed=seed)
            if calibrate is None:
                from .weights import synthetic_patches
                calibrate = synthetic_patches(batch_size, image_size, seed=0)
            # the sampler noise of the calibration call: the fixed one if the caller gave one, else a seeded draw (repeatable)
            # (the counter sampler's own noise, from row 0: range_report)
            noise = None if self._eps_fixed is not None or sampler == "counter" else make_latent_noise(batch_size, latent_dim)
            report = self.range_report(calibrate, eps=noise)
            if report.regime != "parity":
                self.close()
                self.__init__(image_size, batch_size, latent_dim, variant, weights, eps, device, "bf16x3", sampler=sampler,
                              seed=seed)
                if cross != "fp8":
                    report.note = f"cross={cross!r} dropped: it is an option of f16c, and this generator runs bf16x3"
                if head != "separate":
                    report.note = f"head={head!r} dropped: it is an option of f16c, and this generator runs bf16x3"
            self.range = report
            return
        if precision not in _lib.PRECISION_FLAGS:
            raise ValueError(f"unknown precision {precision!r}; expected one of {tuple(_lib.PRECISION_FLAGS) + ('auto',)}")
        self.precision = precision
        self.cross = cross
        self.head = head
        self.range: Optional[RangeReport] = None
        self.image_size, self.batch_size, self.latent_dim, self.variant = image_size, batch_size, latent_dim, variant
        self._lib = _lib.load()
        if not torch.cuda.is_available():
            raise RuntimeError("moonsuperresolution_amd needs a HIP device (MI355X / gfx950); there is no CPU fallback")
        self.device = torch.device("cuda", device)
        cfg = _lib.MsrConfig(image_size, batch_size, latent_dim, _lib.VARIANT_IDS[variant], device,
                             _lib.PRECISION_FLAGS[precision] | _lib.CROSS_FLAGS[cross] | _lib.HEAD_FLAGS[head])
        handle = C.c_void_p()
        rc = self._lib.msr_create(C.byref(cfg), C.byref(handle))
        _lib.raise_for(self._lib, None, rc, "msr_create")
        self._h = handle
        self._eps_mode = eps
        self._eps_fixed: Optional[torch.Tensor] = None
        if isinstance(eps, (int, np.integer)):
            self._eps_fixed = torch.from_numpy(make_latent_noise(batch_size, latent_dim, int(eps))).to(self.device)
        elif eps is not None:
            e = np.ascontiguousarray(eps, dtype=np.float32)
            if e.shape != (batch_size, latent_dim):
                raise ValueError(f"eps must be [{batch_size}, {latent_dim}], got {e.shape}")
            self._eps_fixed = torch.from_numpy(e).to(self.device)
        self.sampler, self.seed = sampler, int(seed)
        self._sampler_calls = 0                                     # calls that took their row ids from this counter
        self._noise: Optional[torch.Tensor] = None                  # sampler="counter": the buffer every call's noise is written to
        if sampler == "counter":
            self._noise = torch.empty((batch_size, latent_dim), dtype=torch.float32, device=self.device)
        self._ctor = dict(image_size=image_size, batch_size=batch_size, latent_dim=latent_dim, variant=variant,
                          eps=eps, device=device, precision=precision, cross=cross, head=head, sampler=sampler, seed=int(seed))
        self._weights: Optional[Mapping[str, np.ndarray]] = None   # what the handle holds now (clone() re-uploads it)
        self.weights_version = 0                                    # bumped by every load(); the tiler's clones follow it
        if isinstance(weights, (int, np.integer)):
            weights = make_weights(variant, image_size, latent_dim, seed=int(weights))
        self.load(weights)

    def clone(self) -> "Generator":
        """A second handle with the weights this handle holds NOW (the last ``load``, not the constructor's), its own
        workspace: for issuing independent calls on another stream, where the latency-bound head of one call overlaps
        the matrix-bound tail of the other.  Sampler and seed are the same; the clone's call counter starts at 0."""
        twin = Generator(weights=self._weights, **self._ctor)
        twin.weights_version = self.weights_version
        twin.range = self.range                  # an "auto" generator's clone is the chosen mode, not calibrated again
        return twin

    # -- weights -----------------------------------------------------------------------------------
    def load(self, weights: Mapping[str, np.ndarray]) -> None:
        """Counterpart of ``gaugan.load(...)`` (process_full_tiles.py:30): takes a name -> array dict."""
        expected = weight_shapes(self.variant, self.image_size, self.latent_dim)
        missing = [k for k in expected if k not in weights]
        if missing:
            raise ValueError(f"missing weights: {missing[:5]}{' ...' if len(missing) > 5 else ''}")
        for name, shape in expected.items():
            a = np.ascontiguousarray(weights[name], dtype=np.float32)
            if tuple(a.shape) != tuple(shape):
                raise ValueError(f"weight {name}: shape {a.shape}, expected {shape}")
            shp = (C.c_int64 * a.ndim)(*a.shape)
            rc = self._lib.msr_load_weight(self._h, name.encode(), a.ctypes.data_as(C.c_void_p), shp, a.ndim)
            _lib.raise_for(self._lib, self._h, rc, f"msr_load_weight({name})")
        self._weights = {name: weights[name] for name in expected}
        self.weights_version += 1

    # -- the call ------------------------------------------------------------------------------------
    def forward_device(self, batch: torch.Tensor, eps: Optional[torch.Tensor] = None,
                       out: Optional[torch.Tensor] = None, gate: Optional[torch.cuda.Event] = None,
                       noise_ids: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Device fast path: ``batch`` [B,S,S,2] float32 on this GPU -> [B,S,S,1] on the GPU (no host copy).

        ``noise_ids`` (sampler="counter" only): int32 / uint32 [B, 3] on this GPU, contiguous — the id of every row's noise
        (msr_sampler_noise); it is read on the current stream.  Without it the rows are (calls * B + b, 0, 0) of this
        instance's call counter.  An explicit ``eps`` is used as given and draws nothing.

        Asynchronous on torch's current stream.  ``gate``: an event recorded at the end of the previous, independent
        call on another handle / stream — the matrix-bound part of this call waits for it, the latency-bound head
        does not (msr_forward_gated)."""
        S, B = self.image_size, self.batch_size
        if tuple(batch.shape) != (B, S, S, 2):
            raise ValueError(f"expected a batch of shape {(B, S, S, 2)} (batch_size is fixed at construction, "
                             f"like the reference's sampler), got {tuple(batch.shape)}")
        if batch.device != self.device or batch.dtype != torch.float32 or not batch.is_contiguous():
            batch = batch.to(device=self.device, dtype=torch.float32).contiguous()
        if out is None:
            out = torch.empty((B, S, S, 1), dtype=torch.float32, device=self.device)
        eps_ptr = None
        if self.variant == "gaugan":
            if eps is None:
                eps = self._eps_fixed
            if eps is None and self.sampler == "counter":
                eps = self._fill_noise(noise_ids)
                noise_ids = None
            elif eps is None:
                eps = torch.randn((B, self.latent_dim), dtype=torch.float32, device=self.device)
            eps = eps.to(device=self.device, dtype=torch.float32).contiguous()
            eps_ptr = eps.data_ptr()
        if noise_ids is not None:
            raise ValueError("noise_ids name the rows of sampler='counter' noise: this call draws none "
                             f"(sampler={self.sampler!r}, variant={self.variant!r}, eps {'given' if eps is not None else 'None'})")
        stream = torch.cuda.current_stream(self.device).cuda_stream
        if gate is not None:
            rc = self._lib.msr_forward_gated(self._h, batch.data_ptr(), eps_ptr, out.data_ptr(), B, stream,
                                             C.c_void_p(gate.cuda_event))
        else:
            rc = self._lib.msr_forward(self._h, batch.data_ptr(), eps_ptr, out.data_ptr(), B, stream)
        _lib.raise_for(self._lib, self._h, rc, "msr_forward")
        return out

    def _fill_noise(self, noise_ids: Optional[torch.Tensor]) -> torch.Tensor:
        """sampler="counter": write this call's noise into the persistent buffer on the current stream and return the buffer.
        The previous call's latent kernel, earlier on the stream this handle's calls are issued on, has read it by then."""
        B = self.batch_size
        ids_ptr, first_row = None, 0
        if noise_ids is not None:
            if tuple(noise_ids.shape) != (B, 3) or noise_ids.dtype not in (torch.int32, torch.uint32) or \
                    noise_ids.device != self.device or not noise_ids.is_contiguous():
                raise ValueError(f"noise_ids must be a contiguous int32 / uint32 tensor of shape {(B, 3)} on {self.device}, got "
                                 f"{noise_ids.dtype} {tuple(noise_ids.shape)} on {noise_ids.device}")
            ids_ptr = noise_ids.data_ptr()
        else:
            first_row = (self._sampler_calls * B) & 0xFFFFFFFF
            self._sampler_calls += 1
        rc = self._lib.msr_sampler_noise(self._h, self.seed, ids_ptr, first_row, self._noise.data_ptr(), B, self.latent_dim,
                                         torch.cuda.current_stream(self.device).cuda_stream)
        _lib.raise_for(self._lib, self._h, rc, "msr_sampler_noise")
        return self._noise

    def reset_sampler(self, calls: int = 0) -> None:
        """sampler="counter": set the call counter, so that the next call without ``noise_ids`` draws rows calls * B .. ."""
        self._sampler_calls = int(calls)

    def __call__(self, batch, training: bool = False) -> np.ndarray:
        """``model(np.array(batch), training=False)`` of process_full_tiles.py:338.

        ``training`` is accepted for signature parity; the SPADE inference path has no mode-dependent layer
        and pix2pix runs its BatchNorm on moving statistics with dropout off (training=False semantics)."""
        if training:
            raise ValueError("this is the inference path: training=True is not supported")
        x = torch.from_numpy(np.ascontiguousarray(np.asarray(batch), dtype=np.float32))
        with torch.cuda.device(self.device):
            y = self.forward_device(x.to(self.device, non_blocking=False))
            return y.cpu().numpy()

    def prepare(self) -> None:
        """Build the launch plan now (workspace, auxiliary stream) instead of at the first call."""
        self.forward_flops()

    def use_graph(self, on: bool = True) -> None:
        """Replay the launch plan as a HIP graph for calls that repeat their (input, noise, output) buffers
        (msr_graph_enable); results identical.  Off by default, and measured in round 3 (bench.py, p50_ms_per_call_b1_graph
        against _eager): on ROCm 7 the replay of this ~90-node plan is 0.07 ms SLOWER per B = 1 call than the eager
        launches (1.96 against 1.89 ms) — the call is bound by ~5 us of dependent-launch latency per small kernel on the
        GPU side, which a graph does not remove.  Kept for hosts whose launch path is slower than this pool's."""
        _lib.raise_for(self._lib, self._h, self._lib.msr_graph_enable(self._h, 1 if on else 0), "msr_graph_enable")

    def last_latent(self) -> np.ndarray:
        z = torch.empty((self.batch_size, self.latent_dim), dtype=torch.float32, device=self.device)
        stream = torch.cuda.current_stream(self.device).cuda_stream
        rc = self._lib.msr_last_latent(self._h, z.data_ptr(), stream)
        _lib.raise_for(self._lib, self._h, rc, "msr_last_latent")
        return z.cpu().numpy()

    def debug_tensor(self, name: str, shape) -> np.ndarray:
        """Copy a named workspace tensor of the last call to the host (per-block parity tests)."""
        out = np.empty(shape, np.float32)
        rc = self._lib.msr_debug_tensor(self._h, name.encode(), out.ctypes.data_as(C.c_void_p), out.size)
        _lib.raise_for(self._lib, self._h, rc, f"msr_debug_tensor({name})")
        return out

    def moment_forms(self) -> dict:
        """{mean tensor name: form} of every planned moments site (msr_debug_moment_forms: A, B, E1/C, E1/D, E2/C, E2/D)."""
        buf = C.create_string_buffer(1 << 16)
        rc = self._lib.msr_debug_moment_forms(self._h, buf, len(buf))
        _lib.raise_for(self._lib, self._h, rc, "msr_debug_moment_forms")
        return dict(line.split(" ") for line in buf.value.decode().splitlines())

    def conv_forms(self) -> list:
        """One dict per planned op, in plan order (msr_debug_conv_forms): kind, tensor names, and for the convs prec, kernel, tile,
        ksplit, wt_frag, no_cross, epi, out_split, ranges and img (the weight image built at upload).  Integers are ints."""
        self.prepare()
        buf = C.create_string_buffer(1 << 18)
        rc = self._lib.msr_debug_conv_forms(self._h, buf, len(buf))
        _lib.raise_for(self._lib, self._h, rc, "msr_debug_conv_forms")
        return parse_conv_forms(buf.value.decode())

    @property
    def head_fused(self) -> bool:
        """Whether the plan took ``head="fused"``: it holds the gather op (the separate head runs at shapes where the last
        residual conv does not run the stream kernel on whole tiles)."""
        return any(op.get("kind") == "head_gather" for op in self.conv_forms())

    # -- dirty-workspace test aids -------------------------------------------------------------------
    def workspace_list(self) -> list:
        """One dict per device buffer of the planned handle (msr_debug_workspace_list): name, kind (ws | scratch | weight |
        table), bytes, zeroed, counted, and r, C, written for the zero-bordered buffers."""
        buf = C.create_string_buffer(1 << 17)
        rc = self._lib.msr_debug_workspace_list(self._h, buf, len(buf))
        _lib.raise_for(self._lib, self._h, rc, "msr_debug_workspace_list")
        return parse_conv_forms(buf.value.decode())

    def fill_workspace(self, what: int, byte: int) -> int:
        """Set every byte of the chosen parts of the workspace to ``byte`` (msr_debug_fill_workspace; ``what``: FILL_WORKSPACE |
        FILL_INTERIOR | FILL_BORDER) and return the number of bytes written.  Synchronises the device."""
        n = C.c_int64()
        rc = self._lib.msr_debug_fill_workspace(self._h, int(what), int(byte), C.byref(n))
        _lib.raise_for(self._lib, self._h, rc, "msr_debug_fill_workspace")
        return n.value

    # -- activation ranges -----------------------------------------------------------------------------
    def range_scan_async(self) -> None:
        """Enqueue a scan of the last call's narrow activation tensors on torch's current stream (msr_range_scan); it must
        be the stream of that call, ahead of the handle's next call.  ``range_read`` collects it."""
        rc = self._lib.msr_range_scan(self._h, torch.cuda.current_stream(self.device).cuda_stream)
        _lib.raise_for(self._lib, self._h, rc, "msr_range_scan")

    def _range_records(self, fn, what: str) -> list:
        from .ops import range_stat_dict
        cap = 256
        arr = (_lib.MsrRangeStat * cap)()
        n = C.c_int32()
        _lib.raise_for(self._lib, self._h, fn(self._h, arr, cap, C.byref(n)), what)
        return [range_stat_dict(arr[i]) for i in range(min(n.value, cap))]

    def range_read(self) -> RangeReport:
        """Wait for the last ``range_scan_async`` and return its RangeReport (with the embed bounds of the gbr ops)."""
        records = self._range_records(self._lib.msr_range_read, "msr_range_read")
        bounds = self._range_records(self._lib.msr_range_embed_bounds, "msr_range_embed_bounds") if records else []
        layers = {}
        if records:
            forms = self.conv_forms()
            for r in records:
                layers[r["producer"]] = forms[r["producer"]].get("wt", "?")
        return RangeReport(records, bounds, layers)

    def range_report(self, batch=None, eps=None) -> RangeReport:
        """Which regime of the narrow formats the last call ran in (RangeReport).  With ``batch`` [B, S, S, 2] (``eps`` as the
        constructor's array form, for "gaugan"), one call is run on it first.  Modes without narrow tensors ("fp32", "bf16x3")
        return an empty report whose regime is "parity".  With sampler="counter" and no ``eps`` that call draws rows 0 .. B - 1
        and leaves the call counter as it was."""
        with torch.cuda.device(self.device):
            if batch is not None:
                x = torch.from_numpy(np.ascontiguousarray(np.asarray(batch), dtype=np.float32)).to(self.device)
                e = None if eps is None else torch.from_numpy(np.ascontiguousarray(eps, dtype=np.float32)).to(self.device)
                calls, self._sampler_calls = self._sampler_calls, 0
                try:
                    self.forward_device(x, eps=e)
                finally:
                    self._sampler_calls = calls
            self.range_scan_async()
            return self.range_read()

    # -- measurement ---------------------------------------------------------------------------------
    def forward_flops(self) -> float:
        v = C.c_double()
        _lib.raise_for(self._lib, self._h, self._lib.msr_forward_flops(self._h, C.byref(v)), "msr_forward_flops")
        return v.value

    def device_bytes(self) -> int:
        v = C.c_int64()
        _lib.raise_for(self._lib, self._h, self._lib.msr_device_bytes(self._h, C.byref(v)), "msr_device_bytes")
        return v.value

    def profile(self, on) -> None:
        """False / 0: off; True / 1: hipEvents around every launch; 2: around runs of conv launches only (cheap)."""
        _lib.raise_for(self._lib, self._h, self._lib.msr_profile_enable(self._h, int(on)), "msr_profile_enable")
        self._lib.msr_profile_reset(self._h)

    def profile_read(self) -> Dict[str, dict]:
        arr = (_lib.MsrKernelStat * 16)()
        n = C.c_int32()
        _lib.raise_for(self._lib, self._h, self._lib.msr_profile_read(self._h, arr, 16, C.byref(n)), "msr_profile_read")
        return {arr[i].name.decode(): dict(launches=arr[i].launches, device_ms=arr[i].device_ms, flops=arr[i].flops,
                                           bytes=arr[i].bytes) for i in range(n.value)}

    def profile_runs(self, ref_event: torch.cuda.Event, family: int = 0):
        """[(start_ms, end_ms, flops, launches)] of the recorded intervals of one kernel family (0 = conv) relative to
        ``ref_event`` (recorded by the caller before the calls)."""
        cap = 1 << 16
        a, b, f = (C.c_double * cap)(), (C.c_double * cap)(), (C.c_double * cap)()
        l = (C.c_int64 * cap)()
        n = C.c_int32()
        rc = self._lib.msr_profile_runs(self._h, C.c_void_p(ref_event.cuda_event), family, a, b, f, l, cap, C.byref(n))
        _lib.raise_for(self._lib, self._h, rc, "msr_profile_runs")
        return [(a[i], b[i], f[i], l[i]) for i in range(n.value)]

    def close(self) -> None:
        if getattr(self, "_h", None):
            self._lib.msr_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
