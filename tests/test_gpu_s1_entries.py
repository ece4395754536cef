"""The preamble and the empty-reduction path that the six stage-1 entries share (csrc/wbx_s1.hpp: s1_begin, s1_operands,
s1_zero_if_empty), straight through the C ABI.  Every call here returns before a launch or issues one memset; the shapes are the
smallest that reach the code: nkey = 2, ndepth = 3, nx = 8, one chunk, one-wave blocks, vec = 1, float32, M = 2, one threshold.
The buffers are real and large enough for a launch of that shape all the same."""
import ctypes as C

import numpy as np
import pytest

from weatherbenchx_amd import _hip

pytestmark = pytest.mark.gpu
NKEY, NDEPTH, NX, M = 2, 3, 8, 2
NPOINT = NKEY * NDEPTH * NX
NOUT = 256  # doubles behind `out`: the largest partial here has 2 * 10 * 8, the rest is guard
FLAGS = {'plain': 0, 'masked': _hip.FLAG_MASKED, 'skipna': _hip.FLAG_SKIPNA}


@pytest.fixture(scope='module')
def ctx():
  assert _hip.is_available(), 'gpu tests need libwbx_hip.so and a HIP device'
  return _hip.default_context(0)


@pytest.fixture(scope='module')
def bufs(ctx):
  rng = np.random.default_rng(0)
  return {'p': ctx.upload(rng.normal(size=M * NPOINT).astype(np.float32)), 't': ctx.upload(rng.normal(size=M * NPOINT).astype(np.float32)),
          'mask': ctx.upload(np.ones(NPOINT, np.uint8)), 'thr': ctx.upload(np.array([0.25]))}


def _plan(nkey=NKEY, ndepth=NDEPTH, nx=NX, x_kept=0, flags=0, block_threads=64):
  plan = _hip.S1PlanStruct()  # (NULL offset tables: every key and row at offset 0, unit x stride)
  plan.nkey, plan.ndepth, plan.nx, plan.x_kept, plan.nchunk, plan.depth_chunk = nkey, ndepth, nx, x_kept, 1, max(ndepth, 1)
  plan.flags, plan.block_threads, plan.vec = flags, block_threads, 1
  for i in (0, 1, 3):
    plan.xstride[i] = 1
  return plan


# entry -> (value lanes, call(lib, handle, plan, dtype, p, t, thr, mask, out))
ENTRIES = {
    'det': (3, lambda lib, h, plan, dt, p, t, thr, mask, out: lib.wbx_det_partial(h, plan, _hip.DET3, dt, p, t, None, mask, out)),
    'ens': (_hip.ENS_LANES, lambda lib, h, plan, dt, p, t, thr, mask, out:
            lib.wbx_ens_partial(h, plan, dt, M, NPOINT, _hip.ENS_SORT, p, t, mask, out)),
    'ens2': (_hip.ENS2_LANES, lambda lib, h, plan, dt, p, t, thr, mask, out:
             lib.wbx_ens2_partial(h, plan, dt, M, NPOINT, M, NPOINT, p, t, mask, out)),
    'cat': (1, lambda lib, h, plan, dt, p, t, thr, mask, out:
            lib.wbx_cat_partial(h, plan, _hip.CAT_EXCEED, dt, 1, M, NPOINT, p, t, thr, mask, out)),
    'cont': (_hip.CONT_CELLS, lambda lib, h, plan, dt, p, t, thr, mask, out: lib.wbx_contingency_partial(h, plan, dt, 1, p, t, thr, mask, out)),
    'erps': (1, lambda lib, h, plan, dt, p, t, thr, mask, out:
             lib.wbx_ens_rps_partial(h, plan, dt, M, NPOINT, 1, thr, thr, 1, p, t, mask, out)),
}

# Exactly one requirement broken -> -1 and the entry's own words.  Pinned elsewhere and not repeated: det / bad plan
# (test_gpu_cabi.test_bad_arguments_return_error_codes), cont / no mask and cont / dtype (test_gpu_contingency.test_refusals),
# erps / no mask and erps / dtype (test_gpu_ens_rps.test_refusals_leave_the_output_untouched).
BAD_PLAN = 'block_threads must be 64, 128 or 256 (got 96)'
NO_MASK = 'WBX_FLAG_MASKED set but mask is NULL'
VIOLATIONS = {
    'det': {'ctx': 'ctx is NULL', 'mask': NO_MASK, 'out': 'output pointer is NULL', 'p': 'predictions pointer is NULL',
            'dtype': 'unknown dtype 7'},
    'ens': {'ctx': 'ctx is NULL', 'plan': BAD_PLAN, 'mask': NO_MASK, 'out': 'output pointer is NULL',
            'p': 'predictions/targets pointer is NULL', 'dtype': 'unknown dtype 7'},
    'ens2': {'ctx': 'ctx is NULL', 'plan': BAD_PLAN, 'mask': NO_MASK, 'out': 'output pointer is NULL',
             'p': 'predictions/targets pointer is NULL', 'dtype': 'unknown dtype 7'},
    'cat': {'ctx': 'ctx is NULL', 'plan': BAD_PLAN, 'mask': NO_MASK, 'out': 'partial_out is NULL', 'p': 'p/t is NULL',
            'dtype': 'unknown dtype 7'},
    'cont': {'ctx': 'wbx_contingency_partial: ctx is NULL', 'plan': BAD_PLAN, 'out': 'wbx_contingency_partial: partial_out is NULL',
             'p': 'wbx_contingency_partial: p/t is NULL'},
    'erps': {'ctx': 'wbx_ens_rps_partial: ctx is NULL', 'plan': BAD_PLAN, 'out': 'wbx_ens_rps_partial: partial_out is NULL',
             'p': 'wbx_ens_rps_partial: p/t is NULL'},
}
VIOLATION_CASES = [(entry, what, text) for entry, table in VIOLATIONS.items() for what, text in table.items()]


def _ptr(buf):
  return C.c_void_p(buf.ptr)


@pytest.mark.parametrize('entry,what,text', VIOLATION_CASES, ids=[f'{e}-{w}' for e, w, _ in VIOLATION_CASES])
def test_one_broken_requirement_is_refused_in_the_entrys_words(ctx, bufs, entry, what, text):
  plan = _plan(flags=_hip.FLAG_MASKED if what == 'mask' else 0, block_threads=96 if what == 'plan' else 64)
  out = ctx.upload(np.full(NOUT, np.nan))
  rc = ENTRIES[entry][1](ctx.lib, None if what == 'ctx' else ctx.handle, C.byref(plan), 7 if what == 'dtype' else _hip.F32,
                         None if what == 'p' else _ptr(bufs['p']), _ptr(bufs['t']), _ptr(bufs['thr']),
                         _ptr(bufs['mask']) if plan.flags and what != 'mask' else None, None if what == 'out' else _ptr(out))
  message = ctx.lib.wbx_last_error().decode()
  assert rc == -1 and text in message, (rc, message)
  assert np.isnan(ctx.download(out.ptr, (NOUT,))).all()


def _call_empty(ctx, bufs, entry, plan, every_pointer_null, mask=True):
  """-> (rc, the NOUT doubles behind `out`, prefilled with NaN; all NaN where `out` is not passed)."""
  out = ctx.upload(np.full(NOUT, np.nan))
  if every_pointer_null:
    rc = ENTRIES[entry][1](ctx.lib, ctx.handle, C.byref(plan), _hip.F32, None, None, None, None, None)
  else:
    rc = ENTRIES[entry][1](ctx.lib, ctx.handle, C.byref(plan), _hip.F32, None, None, _ptr(bufs['thr']),
                           _ptr(bufs['mask']) if plan.flags & _hip.FLAG_MASKED and mask else None, _ptr(out))
  return rc, ctx.download(out.ptr, (NOUT,))


@pytest.mark.parametrize('flags', list(FLAGS))
@pytest.mark.parametrize('x_kept', [0, 1], ids=['x_summed', 'x_kept'])
@pytest.mark.parametrize('entry', list(ENTRIES))
def test_empty_extents_write_exactly_the_partials_zeros(ctx, bufs, entry, x_kept, flags):
  lanes = ENTRIES[entry][0]
  for extent in ({'nkey': 0}, {'ndepth': 0}, {'nx': 0}):
    plan = _plan(x_kept=x_kept, flags=FLAGS[flags], **extent)
    n = C.c_int64(-1)
    _hip.check(ctx.lib.wbx_s1_partial_len(C.byref(plan), lanes, C.byref(n)), 'wbx_s1_partial_len')
    per_key = {'plain': lanes, 'masked': lanes + 1, 'skipna': 2 * lanes}[flags] * (plan.nx if x_kept else 1)
    assert n.value == plan.nkey * per_key, (extent, n.value)
    rc, got = _call_empty(ctx, bufs, entry, plan, every_pointer_null='nkey' in extent)
    if 'nkey' in extent and flags == 'masked' and entry != 'cat':
      # no key and no pointer at all: every entry but the categorical one asks for the mask before it looks at the extent
      assert rc == -1 and NO_MASK in ctx.lib.wbx_last_error().decode(), (extent, rc)
      assert np.isnan(got).all(), extent
      continue
    assert rc == 0, (extent, rc, ctx.lib.wbx_last_error())
    assert (got[:n.value] == 0).all() and np.isnan(got[n.value:]).all(), (extent, n.value, got[:n.value + 2])


def test_only_the_categorical_entry_takes_no_mask_with_an_empty_extent(ctx, bufs):
  """wbx_cat_partial asks for the mask behind its empty return; the other five refuse a NULL mask whatever the extent."""
  for entry, (lanes, _) in ENTRIES.items():
    plan = _plan(ndepth=0, flags=_hip.FLAG_MASKED)
    rc, got = _call_empty(ctx, bufs, entry, plan, every_pointer_null=False, mask=False)
    if entry == 'cat':
      n = NKEY * (lanes + 1)
      assert rc == 0 and (got[:n] == 0).all() and np.isnan(got[n:]).all(), (rc, got[:n + 2])
    else:
      assert rc == -1 and NO_MASK in ctx.lib.wbx_last_error().decode(), (entry, rc)
      assert np.isnan(got).all(), entry
