"""Labelled inputs for the tests of the gate of EnsembleRankedProbabilityScore at threshold fields (multivariate.rps_field_route and
what follows it in `_fused_field_per_variable`): a 3 x 3 (init_time, lead_time) chunk across the end of a leap year on a 4 x 5 grid,
threshold fields over any time dims, and `host_cases()`, every case that must keep the host route.  tests/test_ens_rps_field.py asks
the gate about them without a device; tests/test_gpu_ens_rps_field_api.py runs them through the Aggregator on one."""
import numpy as np

from weatherbenchx_amd import xarray_lite as xr

DAY = np.timedelta64(1, 'D')
LAT, LON = np.linspace(-60, 60, 4), np.arange(5) * 72.0
INITS = np.array(['2020-12-30', '2020-12-31', '2021-01-02'], 'datetime64[ns]')  # (2020 is a leap year: days 365, 366, then 2)
LEADS = np.array([0, 1, 3]) * DAY.astype('timedelta64[ns]')


def field(time_dims: dict, rng, nbin=2):
  """[bin, *time dims, latitude, longitude] thresholds with a NaN, labelled along every dim."""
  dims = ('bin',) + tuple(time_dims) + ('latitude', 'longitude')
  coords = dict(time_dims, bin=np.arange(nbin), latitude=LAT, longitude=LON)
  data = rng.normal(size=tuple(len(coords[d]) for d in dims))
  data[(0,) + (slice(None),) * len(time_dims) + (1, 2)] = np.nan  # (whatever is selected holds one)
  return xr.DataArray(data, dims=dims, coords=coords, name='v')


def chunk(kind):
  if kind == 'init+lead':
    return xr.DataArray(np.zeros((3, 3, 4, 5), np.float32), dims=('init_time', 'lead_time', 'latitude', 'longitude'),
                        coords={'init_time': INITS, 'lead_time': LEADS, 'latitude': LAT, 'longitude': LON}, name='v')
  if kind == 'sparse':  # init_time and lead_time on one dim
    return xr.DataArray(np.zeros((3, 4), np.float32), dims=('index', 'latitude'),
                        coords={'init_time': (('index',), INITS), 'lead_time': (('index',), LEADS[::-1].copy()), 'latitude': LAT}, name='v')
  if kind in ('valid_time', 'time'):
    return xr.DataArray(np.zeros((3, 4, 5), np.float32), dims=(kind, 'latitude', 'longitude'),
                        coords={kind: INITS, 'latitude': LAT, 'longitude': LON}, name='v')
  if kind == 'sparse-time':  # valid_time as a coordinate of another dim
    return xr.DataArray(np.zeros((3, 4), np.float32), dims=('index', 'latitude'), coords={'valid_time': (('index',), INITS[::-1].copy()), 'latitude': LAT}, name='v')
  return xr.DataArray(np.zeros((4, 5), np.float32), dims=('latitude', 'longitude'), coords={'latitude': LAT, 'longitude': LON}, name='v')


def relabelled(da, data=None, **coords):
  """`da` (or `data` on its dims) with some coordinates replaced."""
  return xr.DataArray(np.asarray(da.values) if data is None else data, dims=da.dims,
                      coords=dict({d: da.coords[d].values for d in da.dims if d in da.coords}, **coords), name='v')


def pair(m=4, dtype=np.float32, seed=3):
  """(predictions [number, init_time, lead_time, latitude, longitude], targets) on a grid of quarters: ties with the terciles."""
  rng = np.random.default_rng(seed)
  c = chunk('init+lead')
  cs = {d: c.coords[d].values for d in c.dims}
  quarters = lambda shape: (np.round(rng.normal(size=shape) * 4) / 4).astype(dtype)
  p = xr.DataArray(quarters((m,) + c.shape), dims=('number',) + c.dims, coords=dict(cs, number=np.arange(m)), name='v')
  t = xr.DataArray(quarters(c.shape), dims=c.dims, coords=cs, name='v')
  return p, t


def terciles(seed=5, dtype=np.float32, **kw):
  """[bin, dayofyear, latitude, longitude] on the grid of quarters, strictly increasing along bin, no NaN."""
  f = field({'dayofyear': np.arange(1, 367)}, np.random.default_rng(seed), **kw)
  data = np.asarray(f.values)
  data[np.isnan(data)] = 9.0
  data = np.round(np.sort(data, axis=0) * 4) / 4 + np.arange(data.shape[0]).reshape(-1, 1, 1, 1)
  return relabelled(f, data.astype(dtype))


def host_cases():
  """-> [{what, p, t, pf, tf, kw (of the statistic), by}]: `by` says who declines -- 'route' (rps_field_route) or 'statistic' (what
  `_fused_field_per_variable` looks at afterwards: the values of the field, the frame)."""
  p, t = pair()
  f, g = terciles(), terciles(seed=6)
  plain = xr.DataArray(np.array([0.5, 1.0]), dims=['bin'])
  k17 = xr.DataArray(np.arange(17.0), dims=['bin'])
  no_bin = f.isel(bin=0, drop=True)
  short = f.isel(dayofyear=slice(0, 300))
  nan = relabelled(f)
  nan.values[1, 200, 0, 0] = np.nan  # (a day the chunk does not select)
  falling, shifted = relabelled(f, np.asarray(f.values)[::-1].copy()), relabelled(f, latitude=LAT + 1.0)
  # restate: the restatement of tests/ens_rps_field_cases.py applies to the case as it stands (the whole frame, every bin)
  case = lambda what, p_, t_, pf, tf, by='route', restate=False, **kw: dict(what=what, p=p_, t=t_, pf=pf, tf=tf, kw=kw, by=by, restate=restate)
  return [
      case('skipna_ensemble', p, t, f, f, skipna_ensemble=True, restate=True),
      case('one member, fair', *pair(m=1), f, f),
      case('257 members', *pair(m=257), f, f, restate=True),
      case('ensemble-valued targets', p, relabelled(p), f, f),
      case('integer payloads', relabelled(p, np.asarray(p.values).astype(np.int32)), t, f, f, restate=True),
      case('integer thresholds', p, t, xr.DataArray(np.array([1, 2]), dims=['bin']), xr.DataArray(np.array([1, 2]), dims=['bin']), restate=True),
      case('17 thresholds', p, t, k17, k17, restate=True),
      case('a list on one side', p, t, f, [0.5, 1.0]),
      case('no bin dim', p, t, no_bin, no_bin),
      case('bin labels differ', p, t, f, relabelled(g, bin=np.array([0, 6]))),
      case('labels on one side only', p, t, plain, xr.DataArray(np.array([0.5, 1.0]), dims=['bin'], coords={'bin': [0, 1]})),
      case('K differs', p, t, f, terciles(nbin=3)),
      case('the sides select different thresholds', p, relabelled(t, init_time=INITS + DAY), f, g),
      case('fields that differ in coordinates', p, t, f, relabelled(g, latitude=LAT + 1.0)),
      case('fields that differ in dtype', p, t, f, terciles(seed=6, dtype=np.float64), restate=True),
      case('fields that differ in dims', p, t, f, g.transpose('dayofyear', 'bin', 'latitude', 'longitude'), restate=True),
      case('fields that differ in shape', p, t, f, g.isel(dayofyear=slice(0, 366), latitude=slice(0, 4), longitude=slice(0, 4))),
      case('labels that are not found', p, t, short, short),
      case('the bin dim on an input', p, t, f, f, bin_dim='latitude'),
      case('a field that is not increasing, monotonicity enforced', p, t, falling, falling, by='statistic'),
      case('a field with a NaN, monotonicity enforced', p, t, nan, nan, by='statistic', restate=True),
      case('a frame the field does not broadcast against', p, t, shifted, shifted, by='statistic'),
  ]


def selected(thresholds, chunk_da, frame_dims, bin_dim='bin'):
  """The thresholds every point of `chunk_da`'s frame reads, [frame..., K] (broadcast where the field does not vary), through the
  host route's own selection."""
  from weatherbenchx_amd.metrics import wrappers  # pylint: disable=g-import-not-at-top
  sel = wrappers.select_bin_thresholds_by_time_from_chunk(xr.as_dataarray(thresholds), chunk_da)
  order = [d for d in frame_dims if d in sel.dims] + [bin_dim]
  values = np.asarray(sel.transpose(*order).values, np.float64)
  shape = [chunk_da.sizes[d] if d in sel.dims else 1 for d in frame_dims] + [values.shape[-1]]
  return np.broadcast_to(values.reshape(shape), [chunk_da.sizes[d] for d in frame_dims] + [values.shape[-1]])
