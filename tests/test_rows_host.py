"""Host-side addressing and validation of the row-MLP entry points (fused/rows.py), no GPU needed: what the row kernels K3b / K11 / K10
would be handed for broadcast, row-strided and sliced operands, and the refusals linear_rows makes before it launches anything."""
import pytest
import torch

from py_psnode_amd.fused import rows


def _rows_as_kernel_reads(x2, nrows, rstride, inner, outer, d):
    """The [nrows, d] rows the addressing (row stride, inner rows, outer stride) selects from x2's storage, with a bounds check."""
    if inner == 0:
        size, stride = (nrows, d), (rstride, 1)
        last = (nrows - 1) * rstride + d - 1
    else:
        size, stride = (nrows // inner, inner, d), (outer, rstride, 1)
        last = (nrows // inner - 1) * outer + (inner - 1) * rstride + d - 1
    avail = x2.untyped_storage().nbytes() // x2.element_size() - x2.storage_offset()
    assert last < avail, f"addressing reaches element {last} of {avail}"
    return torch.as_strided(x2, size, stride).reshape(nrows, d)


@pytest.mark.parametrize("case", ["dense", "time_major", "expand_11d", "expand_1bd", "expand_t1d", "col_slice", "rows_2d_expand", "first_rows"])
def test_row_addressing_reads_exactly_the_rows_of_x_inside_its_storage(case):
    """_row_addressing never reports a row stride its tensor does not have: a stride-0 (broadcast) row dimension -- `expand` of
    [1, 1, d], [1, B, d], [T, 1, d] -- is copied once, not read as if its rows were d apart (the kernel would read T * B rows out of
    a buffer of d floats)."""
    T, B, d = 7, 5, 6
    g = torch.Generator().manual_seed(3)
    x = {"dense": lambda: torch.randn(T, B, d, generator=g),
         "time_major": lambda: torch.randn(B, T, d, generator=g).permute(1, 0, 2),
         "expand_11d": lambda: torch.randn(1, 1, d, generator=g).expand(T, B, d),
         "expand_1bd": lambda: torch.randn(1, B, d, generator=g).expand(T, B, d),
         "expand_t1d": lambda: torch.randn(T, 1, d, generator=g).expand(T, B, d),
         "col_slice": lambda: torch.randn(T, B, d + 3, generator=g)[..., 1:1 + d],
         "rows_2d_expand": lambda: torch.randn(1, d, generator=g).expand(T * B, d),
         "first_rows": lambda: torch.randn(B, T, d, generator=g)[:, 0]}[case]()
    x2, nrows, rstride, inner, outer = rows._row_addressing(x)
    assert nrows == x.numel() // d and rstride >= d
    assert torch.equal(_rows_as_kernel_reads(x2, nrows, rstride, inner, outer, d), x.reshape(-1, d))


@pytest.mark.parametrize("shape,stride", [((12, 8), (0, 1)), ((12, 8), (0, 0)), ((12, 7), (0, 1)), ((12, 8), (9, 1)), ((12, 8), (2, 1)),
                                          ((1, 8), (0, 1)), ((12, 1), (0, 0))])
def test_row_operands_handed_to_kernels_have_row_stride_at_least_their_width(shape, stride):
    """_rows_arg / _ld (linear_rows' X and Hh, every grad_out of the row backward kernels) and _pad4 (K10's operands): the rows of a
    broadcast upstream gradient -- strides (0, 1) after `(y.sum((0, 1)) * w).sum()`, (0, 0) after `y.sum()` -- or of an overlapping
    view are copied, never passed with ld = 0 or ld < width."""
    base = torch.randn(200)
    t2 = torch.as_strided(base, shape, stride)
    a = rows._rows_arg(t2)
    assert torch.equal(a, t2) and (a.shape[1] == 1 or a.stride(1) == 1) and rows._ld(a) >= a.shape[1]
    p = rows._pad4(t2)
    assert p.shape == (shape[0], (shape[1] + 3) // 4 * 4) and p.stride(1) == 1 and rows._ld(p) >= p.shape[1] and rows._ld(p) % 4 == 0
    assert torch.equal(p[:, :shape[1]], t2) and not p[:, shape[1]:].any()


def test_linear_rows_refuses_foreign_parameters_before_any_launch():
    """dtype and width checks of W, bias (and hh) happen on the host, before the kernel is asked anything."""
    x = torch.randn(33, 36)
    W, b = torch.randn(20, 36), torch.randn(20)
    with pytest.raises(TypeError):
        rows.linear_rows(x.double(), W, b)
    with pytest.raises(TypeError):
        rows.linear_rows(x, W.double(), b)
    with pytest.raises(TypeError):
        rows.linear_rows(x, W, b.half())
    with pytest.raises(ValueError, match="width"):
        rows.linear_rows(torch.randn(33, 40), W, b)
    with pytest.raises(ValueError, match="width"):
        rows.linear_rows(x, W, b, transposed=True)
    with pytest.raises(ValueError, match="elements"):
        rows.linear_rows(x, W, torch.randn(21))
    with pytest.raises(TypeError):
        rows.linear_rows(x, W, None, epi=2, hh=torch.randn(33, 20).double())
    with pytest.raises(ValueError):
        rows.linear_rows(x, W, b, out=torch.empty(33, 19))


def test_row_mlp_predicates_refuse_foreign_parameters():
    """wide_rows_class / rows_layers_of: parameters that are not fp32 on the input's HIP device never reach a row kernel."""
    import torch.nn as nn
    seq = nn.Sequential(nn.Linear(8, 36), nn.ELU(), nn.Linear(36, 8))
    layers = [(seq[0].weight, seq[0].bias), (seq[2].weight, seq[2].bias)]
    assert not rows.wide_rows_class(layers)                        # CPU parameters
    assert rows.rows_layers_of(seq, torch.randn(4, 8), allow_grad=True) is None
    assert not rows._params_f32_on([(w.double(), b) for w, b in layers], torch.device("cuda", 0))
