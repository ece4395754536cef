"""SEEPS without a device: the score table (categorical.seeps_score_table) and the per-point restatement of wbx_seeps_partial
(tests/seeps_cases.py) against the host route `SEEPS._one` bit for bit, what the Python layer sends to the launch, and the gate of the
fused route."""
import os

import numpy as np
import pytest

import fake_device
import seeps_cases as SC
from weatherbenchx_amd import _hip
from weatherbenchx_amd import aggregation
from weatherbenchx_amd import engine
from weatherbenchx_amd import lazy
from weatherbenchx_amd import planner
from weatherbenchx_amd import replay
from weatherbenchx_amd import xarray_lite as xr
from weatherbenchx_amd.metrics import categorical

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V = SC.VAR


def _stat(clim, **kw):
  return categorical.SEEPS([V], clim, kw.pop('dry_threshold_mm', SC.DRY_MM), kw.pop('min_p1', SC.MIN_P1), kw.pop('max_p1', SC.MAX_P1))


def _host(stat, pred, targ):
  with np.errstate(all='ignore'):
    return stat._one(xr.as_dataarray(pred[V]), xr.as_dataarray(targ[V]), V, stat._dry_threshold_mm[0], stat._min_p1[0], stat._max_p1[0])  # pylint: disable=protected-access


def _table_of(clim, min_p1=SC.MIN_P1, max_p1=SC.MAX_P1):
  with np.errstate(all='ignore'):
    p1 = xr.as_dataarray(clim[f'{V}_seeps_dry_fraction']).mean(('hour', 'dayofyear'))
  table = categorical.seeps_score_table(p1, min_p1, max_p1)
  return table.reshape((9, 1, 1) + table.shape[2:]), np.asarray(p1.values)


# ---- the table and the restatement ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('clim_dtype', [None, np.float32], ids=['clim_as_inputs', 'clim_float32'])
@pytest.mark.parametrize('dtype', [np.float32, np.float64], ids=['float32', 'float64'])
def test_table_and_restatement_are_the_host_route_bit_for_bit(dtype, clim_dtype):
  for seed, mask_on in ((5, None), (6, 'targets'), (7, 'predictions')):
    pred, targ, clim, wet = SC.labelled_case(dtype, seed, mask_on=mask_on, clim_dtype=clim_dtype)
    host = _host(_stat(clim), pred, targ)
    table9, p1 = _table_of(clim)
    assert table9.dtype == np.float64 and p1.dtype == (clim_dtype or dtype)
    p, t = pred[V].values, targ[V].values
    compare = np.result_type(dtype, wet.dtype)  # a float64 field against float32 thresholds is compared in float64, as NumPy does
    values = SC.point_values(p, t, wet, table9, SC.DRY_THRESHOLD, compare)
    SC.assert_case_is_telling(p, t, wet, values, SC.DRY_THRESHOLD, compare)
    assert host.dims == SC.DIMS and SC.same_numbers(values, host.values), (seed, mask_on)
    # the special places are all there, and the host route's mask is theirs and the side's
    for special in (0.0, 1.0, SC.MIN_P1, SC.MAX_P1, np.nextafter(SC.MIN_P1, -1), np.nextafter(SC.MAX_P1, 2)):
      assert (p1 == p1.dtype.type(special)).any(), special
    assert np.isnan(p1).any()
    with np.errstate(invalid='ignore'):
      in_range = (p1 >= SC.MIN_P1) & (p1 <= SC.MAX_P1)
    side = pred[V] if mask_on == 'predictions' else targ[V]
    want_mask = in_range[None, None] & np.asarray(side.coords['mask'].values) if mask_on else in_range  # (the place dims alone)
    np.testing.assert_array_equal(np.asarray(host.coords['mask'].values), want_mask)


@pytest.mark.parametrize('dtype', [np.float32, np.float64], ids=['float32', 'float64'])
def test_on_tensors_the_table_is_the_tensor_route_bit_for_bit(dtype):
  """torch rounds `3 / (1 - p1)` as 3 * (1 / (1 - p1)): the table is evaluated on whatever holds the dry fractions, so it is the host
  route of that library, which is not NumPy's to the last bit."""
  import torch  # pylint: disable=g-import-not-at-top
  pred, targ, clim, wet = SC.labelled_case(dtype, 11, mask_on='targets')
  tensor = lambda da: xr.DataArray(torch.as_tensor(np.asarray(da.values)), dims=da.dims, coords=dict(da.coords))
  pred_t, targ_t, clim_t = {V: tensor(pred[V])}, {V: tensor(targ[V])}, {k: tensor(v) for k, v in clim.items()}
  host = _host(_stat(clim_t), pred_t, targ_t)
  assert torch.is_tensor(host.data) and host.data.dtype == torch.float64
  table9, _ = _table_of(clim_t)
  values = SC.point_values(pred[V].values, targ[V].values, wet, table9, SC.DRY_THRESHOLD, dtype)
  assert SC.same_numbers(values, np.asarray(host.values))
  assert not SC.same_numbers(table9, _table_of(clim)[0])  # (the reason: NumPy's table differs in last bits)


@pytest.mark.parametrize('dtype', [np.float32, np.float64], ids=['float32', 'float64'])
def test_every_cell_of_every_special_place(dtype):
  """One latitude per dry fraction -- 0, 1, NaN, both ends of a range that holds 0 and 1, just outside, inside -- and nine longitudes
  that walk the cells: the table's entry is `_one`'s value, 0 * inf and all."""
  for lo, hi in ((SC.MIN_P1, SC.MAX_P1), (0.0, 1.0)):
    special = np.array([0.0, 1.0, np.nan, lo, hi, np.nextafter(lo, -1), np.nextafter(hi, 2), -2.0, 0.1, 0.85, 0.5], dtype)
    n = special.size
    lat, lon = np.arange(n) * 1.0, np.arange(9) * 10.0
    cs = {'dayofyear': np.arange(1, 367), 'hour': np.array([0, 6, 12, 18]), 'latitude': lat, 'longitude': lon}
    wet = np.full((366, 4, n, 9), 0.005, dtype)
    p1 = np.broadcast_to(special[:, None], (1, 1, n, 9)).copy()
    clim = {f'{V}_seeps_threshold': xr.DataArray(wet, dims=tuple(cs), coords=cs),
            f'{V}_seeps_dry_fraction': xr.DataArray(p1, dims=tuple(cs), coords=dict(cs, dayofyear=[1], hour=[0]))}
    by_cat = np.array([0.0001, 0.002, 0.02], dtype)
    c2 = {'init_time': np.array(['2020-03-01T00'], 'datetime64[ns]'), 'lead_time': np.array([6], 'timedelta64[h]').astype('timedelta64[ns]'),
          'latitude': lat, 'longitude': lon}
    p = np.broadcast_to(by_cat[np.arange(9) // 3], (1, 1, n, 9)).copy()
    t = np.broadcast_to(by_cat[np.arange(9) % 3], (1, 1, n, 9)).copy()
    pred = {V: xr.DataArray(p, dims=SC.DIMS, coords=c2)}
    targ = {V: xr.DataArray(t, dims=SC.DIMS, coords=c2)}
    host = _host(_stat(clim, min_p1=lo, max_p1=hi), pred, targ)
    table9, _ = _table_of(clim, lo, hi)
    got = np.stack([table9[c, 0, 0, :, c] for c in range(9)], axis=-1)  # longitude c holds cell c
    assert SC.same_numbers(got, np.asarray(host.values)[0, 0]), (lo, hi)
    if lo == 0.0:  # a dry fraction of 0 or 1 inside the range: 0 * inf makes the whole row NaN, the diagonal too
      assert np.isnan(got[0]).all() and np.isnan(got[1]).all()
    assert (got[-1, [0, 4, 8]] == 0).all() and got[-1, 1] == 0.5 * (1 / (1 - dtype(0.5)))


def test_the_float32_dry_threshold_itself_is_dry():
  at = np.float32(SC.DRY_THRESHOLD)
  assert float(at) > SC.DRY_THRESHOLD  # ... so a float64 comparison calls it light
  assert SC.categories([at], [0.005], SC.DRY_THRESHOLD, np.float32)[0] == SC.DRY
  assert SC.categories([float(at)], [0.005], SC.DRY_THRESHOLD, np.float64)[0] == SC.LIGHT
  lo, _, hi = SC.next_to(SC.DRY_THRESHOLD, np.float32)
  np.testing.assert_array_equal(SC.categories([lo, at, hi, -0.0, np.inf, -np.inf, np.nan], [0.005] * 7, SC.DRY_THRESHOLD, np.float32),
                                [SC.DRY, SC.DRY, SC.LIGHT, SC.DRY, SC.HEAVY, SC.DRY, SC.NONE])
  np.testing.assert_array_equal(SC.categories([lo, hi, np.inf], [np.nan] * 3, SC.DRY_THRESHOLD, np.float32), [SC.DRY, SC.NONE, SC.NONE])
  # and so says the host route: forecast float32(d), observed heavy at a place with p1 = 0.5 costs 0.5 * 4 / (1 - p1) = 4
  for dtype, want in ((np.float32, 4.0), (np.float64, 3.0)):  # (as float64 the same number is light: 0.5 * 3 / (1 - p1))
    cs = {'dayofyear': np.arange(1, 367), 'hour': np.array([0, 6, 12, 18]), 'latitude': [0.0], 'longitude': [0.0]}
    clim = {f'{V}_seeps_threshold': xr.DataArray(np.full((366, 4, 1, 1), 0.005, dtype), dims=tuple(cs), coords=cs),
            f'{V}_seeps_dry_fraction': xr.DataArray(np.full((1, 1, 1, 1), 0.5, dtype), dims=tuple(cs), coords=dict(cs, dayofyear=[1], hour=[0]))}
    c2 = {'init_time': np.array(['2020-03-01T00'], 'datetime64[ns]'), 'lead_time': np.array([6], 'timedelta64[h]').astype('timedelta64[ns]'),
          'latitude': [0.0], 'longitude': [0.0]}
    pred = {V: xr.DataArray(np.full((1, 1, 1, 1), at, dtype), dims=SC.DIMS, coords=c2)}
    targ = {V: xr.DataArray(np.full((1, 1, 1, 1), 0.02, dtype), dims=SC.DIMS, coords=c2)}
    assert float(np.asarray(_host(_stat(clim), pred, targ).values).reshape(())) == want


# ---- what the Python layer sends ------------------------------------------------------------------------------------------------------
def test_the_place_block_and_the_table_layout():
  sizes = {'latitude': 3, 'longitude': 4, 'level': 1}
  assert engine.place_block({'latitude': 4, 'longitude': 1}, sizes, ('latitude', 'longitude')) == (('latitude', 'longitude'), 12)
  assert engine.place_block({'latitude': 1, 'longitude': 3}, sizes, ('latitude', 'longitude')) == (('longitude', 'latitude'), 12)
  assert engine.place_block({'latitude': 4, 'longitude': 1, 'level': 99}, sizes, ('level', 'latitude', 'longitude'))[1] == 12
  assert engine.place_block({'latitude': 16, 'longitude': 1}, sizes, ('latitude', 'longitude')) is None  # `hour` between them
  assert engine.place_block({'latitude': 8, 'longitude': 2}, sizes, ('latitude', 'longitude')) is None  # the places are outermost
  table = np.arange(9.0 * 12).reshape(3, 3, 3, 4)
  uploads = []
  ctx = type('Ctx', (), {'device_id': 0, 'upload': lambda self, a: uploads.append(np.array(a)) or type('Buf', (), {'ptr': len(uploads)})()})()
  dev = lambda **st: type('Dev', (), {'layout': planner.InputLayout(strides=st)})()
  cat = {'dry_threshold': 0.00025, 'table': table, 'place_dims': ('latitude', 'longitude'), 'device_tables': {}}
  nl, ens, args = engine._seeps_operands(ctx, [None, None, dev(dayofyear=48, hour=12, latitude=4, longitude=1), None], 0, None, cat, None)  # pylint: disable=protected-access
  assert (nl, ens, args.dry, args.cell_stride) == (1, None, 0.00025, 12) and uploads[0].shape == (9, 3, 4)
  np.testing.assert_array_equal(uploads[0], table.reshape(9, 3, 4))
  engine._seeps_operands(ctx, [None, None, dev(dayofyear=48, hour=12, latitude=4, longitude=1), None], 0, None, cat, None)  # pylint: disable=protected-access
  assert len(uploads) == 1  # once per device and layout
  _, _, args = engine._seeps_operands(ctx, [None, None, dev(dayofyear=48, hour=12, latitude=1, longitude=3), None], 0, None, cat, None)  # pylint: disable=protected-access
  np.testing.assert_array_equal(uploads[1], table.reshape(9, 3, 4).transpose(0, 2, 1))  # longitude outermost: the climatology's order
  assert args.cell_stride == 12 and args.table.ptr == 2
  with pytest.raises(ValueError, match='not one dense block'):
    engine._seeps_operands(ctx, [None, None, dev(dayofyear=48, hour=4, latitude=16, longitude=1), None], 0, None, cat, None)  # pylint: disable=protected-access
  name, call = engine._KINDS['seeps'].call(['p', 't', 'w', 'm'], 'out', _hip.F32, 0, None, args)  # pylint: disable=protected-access
  assert name == 'wbx_seeps_partial' and call[0] == _hip.F32 and call[1].value == 0.00025 and call[2:5] == ('p', 't', 'w')
  assert call[5].value == 2 and call[6:] == (12, 'm', 'out') and len(call) + 2 == 11  # (ctx and plan in front)


def test_a_recorded_call_carries_a_double_as_its_bits():
  import ctypes as C  # pylint: disable=g-import-not-at-top
  for v in (0.00025, -0.0, float('inf')):
    assert replay._arg64(C.c_double(v), []) == int(np.float64(v).view(np.uint64)) == replay._arg64(v, [])  # pylint: disable=protected-access
  assert _hip.FN_IDS['wbx_seeps_partial'] == 27 and 'wbx_seeps_partial' in _hip.EXPORTED_SYMBOLS


def test_the_rotation_of_the_raw_abi_test_reaches_every_setting():
  """tests/test_gpu_seeps.py walks the row lengths while its other settings rotate (seeps_cases.rotation): every setting is met, in
  the combinations that matter."""
  seen = []
  for m in range(SC.N_MODES):
    for f64 in (0, 1):
      for j in range(len(SC.TABLE_KINDS)):
        for i, nx in enumerate(SC.WIDTHS):
          r = SC.rotation(i + 7 * j, 3 * m + f64)
          seen.append(dict(r, nx=nx, vec=SC.launch_vec(r, nx)))
  for key, all_of in (('nkey', {1, 2}), ('nrow', {1, 3}), ('x_kept', {True, False}), ('two_chunks', {True, False}), ('gather', set(SC.GATHERS)),
                      ('transposed', {True, False}), ('threads', {256, 128, 64}), ('vec', {1, 4})):
    assert {r[key] for r in seen} == all_of, key
  assert {(r['x_kept'], r['vec']) for r in seen} == {(True, 1), (True, 4), (False, 1), (False, 4)}
  assert {(r['gather'], r['transposed']) for r in seen} == {(g, tr) for g in SC.GATHERS for tr in (True, False)}
  assert {r['nx'] for r in seen if not r['x_kept']} == set(SC.WIDTHS) == {r['nx'] for r in seen if r['x_kept']}


def test_the_threshold_check_decides_in_the_comparison_type_where_the_thresholds_lie():
  """float32(0.00025) is above 0.00025 as float64 and equal to the dry threshold as float32: wet thresholds that hold it pass under
  float64 fields and are declined under float32 fields; one ulp below it they are declined under both.  NumPy arrays and tensors."""
  import torch  # pylint: disable=g-import-not-at-top
  _, _, clim, _ = SC.labelled_case(np.float32, 21)
  wet, dry = clim[f'{V}_seeps_threshold'], clim[f'{V}_seeps_dry_fraction']
  at = np.float32(SC.DRY_THRESHOLD)
  for value, ok64, ok32 in ((at, True, False), (np.nextafter(at, np.float32(0)), False, False), (np.nextafter(at, np.float32(1)), True, True)):
    low = np.array(wet.values)
    low[5, 2, 1, 3] = value
    for holder in (low, torch.as_tensor(low)):
      da = xr.DataArray(holder, dims=wet.dims, coords=dict(wet.coords))
      places = lambda dtype: categorical.SEEPS._fused_places(da, dry, wet.dims[2:], dtype, SC.DRY_MM, SC.MIN_P1, SC.MAX_P1)  # pylint: disable=protected-access
      with np.errstate(all='ignore'):
        assert (places('float64') is not None) == ok64 and (places('float32') is not None) == ok32, (value, type(holder))
  low = np.array(wet.values, np.float64)
  low[5, 2, 1, 3] = SC.DRY_THRESHOLD
  da = xr.DataArray(low, dims=wet.dims, coords=dict(wet.coords))
  with np.errstate(all='ignore'):
    assert categorical.SEEPS._fused_places(da, dry, wet.dims[2:], 'float64', SC.DRY_MM, SC.MIN_P1, SC.MAX_P1) is None  # pylint: disable=protected-access


# ---- the gate ---------------------------------------------------------------------------------------------------------------------------
class _Ctx(_hip.Context):  # a context the gate may ask: nothing is launched on it
  def __init__(self):  # pylint: disable=super-init-not-called
    self.lib = type('Lib', (), {'wbx_seeps_partial': staticmethod(lambda *a: 0)})()
    self.device_id = 0

  def __del__(self):
    pass


def _is_fused(stat):
  return isinstance(stat, lazy.LazyStatistic) and stat._group.kind == 'seeps'  # pylint: disable=protected-access


def _same(a, b):
  assert a.dims == b.dims and a.name == b.name and a.dtype == b.dtype and a.shape == b.shape
  assert SC.same_numbers(np.asarray(a.values), np.asarray(b.values))
  assert set(a.coords) == set(b.coords)
  for k in a.coords:
    assert a.coords[k].dims == b.coords[k].dims, k
    np.testing.assert_array_equal(np.asarray(a.coords[k].values), np.asarray(b.coords[k].values))


@pytest.mark.parametrize('dtype', [np.float32, np.float64], ids=['float32', 'float64'])
def test_the_gate_takes_the_plain_case_and_labels_it_as_the_host_route(monkeypatch, dtype):
  monkeypatch.setattr(_hip, 'default_context', _Ctx)
  monkeypatch.setattr(lazy, 'FUSED_SEEPS', True)
  for mask_on, clim_dtype in ((None, None), ('targets', None), ('predictions', np.float32)):
    pred, targ, clim, _ = SC.labelled_case(dtype, 11, mask_on=mask_on, clim_dtype=clim_dtype)
    stat = _stat(clim)
    with np.errstate(all='ignore'):
      got = stat.compute(pred, targ)[V]
    assert _is_fused(got) and got.is_lazy and 'mask' in got.coords and got.dtype == np.float64
    grp = got._group  # pylint: disable=protected-access
    assert grp.clim is not None and grp.clim.source is clim[f'{V}_seeps_threshold'] and len(grp.inputs_and_func()[0]) == 3
    assert grp.cat['table'].shape == (3, 3, 6, 8) and grp.cat['dry_threshold'] == SC.DRY_THRESHOLD
    np.testing.assert_array_equal(np.asarray(grp.mask.values), np.asarray(got.coords['mask'].values))
    again = stat.compute(pred, targ)[V]
    assert again._group is grp and again._group.cat['device_tables'] is grp.cat['device_tables']  # pylint: disable=protected-access
    host = _host(stat, pred, targ)
    assert got.is_lazy
    with np.errstate(all='ignore'):
      _same(got, host)  # (reading .values is the host route)
  # the next chunk of the same statistic shares the table and its device copies
  other, targ2, _, _ = SC.labelled_case(dtype, 11, first_day='2020-06-01T00')
  with np.errstate(all='ignore'):
    nxt = stat.compute(other, targ2)[V]
  assert _is_fused(nxt) and nxt._group is not grp and nxt._group.cat['table'] is grp.cat['table']  # pylint: disable=protected-access
  assert nxt._group.cat['device_tables'] is grp.cat['device_tables']  # pylint: disable=protected-access


def test_the_gate_declines_every_fallback_condition_without_a_device(monkeypatch):
  monkeypatch.setattr(_hip, 'default_context', _Ctx)
  monkeypatch.setattr(lazy, 'FUSED_SEEPS', True)
  for why, (a, b, cl) in SC.decline_cases().items():
    stat = _stat(cl)
    try:
      want = _host(stat, a, b)
    except (KeyError, ValueError) as e:  # the host route itself refuses: so does compute()
      with pytest.raises(type(e)):
        stat.compute(a, b)
      continue
    with np.errstate(all='ignore'):
      got = stat.compute(a, b)[V]
    assert not isinstance(got, lazy.LazyStatistic), why
    _same(got, want)
  # masks on both sides: the host route's error
  pred, targ, clim, _ = SC.labelled_case(np.float32, 21, mask_on='targets')
  both = {V: pred[V].assign_coords(mask=targ[V].coords['mask'])}
  with pytest.raises(ValueError, match='Both predictions and targets have masks'):
    _stat(clim).compute(both, targ)
  # the switch
  monkeypatch.setattr(lazy, 'FUSED_SEEPS', False)
  with np.errstate(all='ignore'):
    got = _stat(clim).compute(pred, targ)[V]
  assert not isinstance(got, lazy.LazyStatistic)
  _same(got, _host(_stat(clim), pred, targ))


def test_a_library_without_the_symbol_or_no_device_keep_the_host_route(monkeypatch):
  class Old(_Ctx):
    def __init__(self):  # pylint: disable=super-init-not-called
      self.lib = type('Lib', (), {})()
  monkeypatch.setattr(lazy, 'FUSED_SEEPS', True)
  pred, targ, clim, _ = SC.labelled_case(np.float32, 11)
  monkeypatch.setattr(_hip, 'default_context', Old)
  with np.errstate(all='ignore'):
    assert not _is_fused(_stat(clim).compute(pred, targ)[V])

  def no_device(*a, **k):
    raise _hip.WbxUnavailableError('no device')
  monkeypatch.setattr(_hip, 'default_context', no_device)
  with np.errstate(all='ignore'):
    assert not _is_fused(_stat(clim).compute(pred, targ)[V])
  assert not engine.seeps_available(object()) and engine.seeps_available(_Ctx())


def test_the_emulated_context_keeps_the_host_route(monkeypatch):
  """The plan interpreter's context is no _hip.Context, so nothing asks it for the new launch: SEEPS through the Aggregator is the
  restatement's masked mean."""
  engine.clear_caches()
  fake_device.install(monkeypatch)
  monkeypatch.setattr(lazy, 'FUSED_SEEPS', True)
  log = []
  monkeypatch.setattr(engine, 'S1_EVENT_LOG', log)
  pred, targ, clim, wet = SC.labelled_case(np.float64, 10, mask_on='targets')
  stat = _stat(clim)
  with np.errstate(all='ignore'):
    stats = {stat.unique_name: stat.compute(pred, targ)}
    assert not isinstance(stats[stat.unique_name][V], lazy.LazyStatistic)
    out = aggregation.Aggregator(reduce_dims=list(SC.DIMS), masked=True).aggregate_statistics(stats)
  assert not [e for e in log if e['kind'] == 'seeps']
  table9, _ = _table_of(clim)
  values = SC.point_values(pred[V].values, targ[V].values, wet, table9, SC.DRY_THRESHOLD, np.float64)
  mask = np.asarray(stats[stat.unique_name][V].coords['mask'].values)
  got = out.mean_statistics()[stat.unique_name][V]
  np.testing.assert_allclose(float(np.asarray(got.values)), np.where(mask, values, 0).sum() / mask.sum(), rtol=1e-12)
  engine.clear_caches()


def test_the_switch_reads_the_environment_and_the_readme_documents_it():
  assert lazy.FUSED_SEEPS == (os.environ.get('WBX_FUSED_SEEPS', '1') != '0')
  with open(os.path.join(ROOT, 'README.md')) as f:
    readme = f.read()
  row = [line for line in readme.splitlines() if line.startswith('| `WBX_FUSED_SEEPS` |')]
  assert len(row) == 1 and 'wbx_seeps_partial' in row[0] and 'tools/bench_seeps.py' in row[0]
  assert 'SEEPS' in [line for line in readme.splitlines() if line.startswith('| hot kernels |')][0]
