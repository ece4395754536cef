"""`xarray_lite._where` / `DataArray.where` on tensor payloads promote like NumPy: a float fill of a Boolean or integer tensor gives a
floating-point result (a NaN fill cannot live in a Boolean tensor, where it used to turn into True, nor in an integer one), while
integer fills and floating-point tensors keep their type."""
import numpy as np
import pytest

from weatherbenchx_amd import xarray_lite as xr

torch = pytest.importorskip('torch')

COND = np.array([True, False, True, False])
PAYLOADS = {'bool': np.array([True, True, False, False]), 'int32': np.array([3, -4, 0, 7], np.int32), 'int64': np.array([3, -4, 0, 7], np.int64),
            'float32': np.array([1.5, -2.0, 0.0, np.inf], np.float32), 'float64': np.array([1.5, -2.0, 0.0, np.inf])}


@pytest.mark.parametrize('fill', [np.nan, 0.5, np.float32(2.0), np.float64(-1.0)], ids=['nan', 'half', 'float32', 'float64'])
@pytest.mark.parametrize('kind', list(PAYLOADS))
def test_a_float_fill_promotes_like_numpy(kind, fill):
  a = PAYLOADS[kind]
  want = np.where(COND, a, fill)
  got = xr._where(torch.as_tensor(COND), torch.as_tensor(a), fill)  # pylint: disable=protected-access
  assert got.is_floating_point()
  np.testing.assert_array_equal(got.numpy().astype(np.float64), want.astype(np.float64))
  if a.dtype.kind in 'bi':
    assert got.dtype == torch.float64  # (what NumPy gives for a Python float; a float32 scalar fill is widened too: no value changes)
    assert want.dtype == np.float64 or isinstance(fill, np.float32)
  else:
    assert got.dtype == torch.as_tensor(a).dtype  # a floating-point tensor keeps its type
  if isinstance(fill, float) and np.isnan(fill):
    assert np.isnan(got.numpy()[~COND]).all() and not np.isnan(got.numpy()[COND]).any()


@pytest.mark.parametrize('kind', ['bool', 'int32', 'int64'])
def test_an_integer_fill_keeps_the_type(kind):
  a = PAYLOADS[kind]
  got = xr._where(torch.as_tensor(COND), torch.as_tensor(a), 0)  # pylint: disable=protected-access
  assert got.dtype == torch.as_tensor(a).dtype
  np.testing.assert_array_equal(got.numpy(), np.where(COND, a, 0).astype(a.dtype))


def test_where_of_a_boolean_labelled_array_keeps_nan_on_both_payload_kinds():
  x = np.array([0.5, np.nan, 2.0, -1.0], np.float32)
  for payload in (x, torch.as_tensor(x)):
    da = xr.DataArray(payload, dims=['i'])
    out = (da > 1.0).where(~da.isnull()).astype(np.float32)
    values = out.values
    values = np.asarray(values.cpu()) if xr._is_torch(values) else np.asarray(values)  # pylint: disable=protected-access
    np.testing.assert_array_equal(values, np.array([0.0, np.nan, 1.0, 0.0], np.float32))
    assert values.dtype == np.float32
