"""oracle/ — TEST INFRASTRUCTURE ONLY.

CPU checkers for the gapped-k-mer kernel path. Only ``tests/``, ``__graft_entry__.smoke()`` and the
``cpu_baseline`` leg of ``bench.py`` may import this package; the product (``fastsk_amd``) never
does and fails loudly when its HIP library is missing.

Two checkers live here:

* ``oracle.port``  – ``liboracle.so``: our own plain-C restatement of the reference algorithm
  (``fastsk_oracle.c``; every function cites the reference file:line it follows).
* ``oracle.ref``   – ``_ref/libfastsk_ref.so``: the real reference compiled from its own sources
  (see ``Makefile`` / ``ref_harness.cpp``). Present when built in the container that holds
  ``/root/reference``; the prebuilt file travels to the GPU box.

``port.raw_counts`` is a 32-BIT reference within one call: like the reference's ``unsigned int Ks`` its cells wrap
mod 2^32 while the combinations of a call are summed, and widen to 64 bits only between calls. Inputs where a cell of
one call reaches 2^32 (15 combinations over a sequence of 20,000 windows; one combination over 65,536 equal windows,
which returns 0) need a 64-bit reference: ``tests/wide_cells_cases.py:counts_by_definition``, which this oracle proves
one combination at a time, modulo 2^32.

Parity status: PINNED. ``liboracle.so`` is checked bit-for-bit against ``libfastsk_ref.so`` and
against the committed golden vectors in ``tests/golden`` (generated from the compiled reference by
``tests/make_golden.py``).
"""
from . import loader  # noqa: F401
from .loader import port, ref, have_ref, build  # noqa: F401
