"""dsss_mosaic_grid: the host arithmetic that turns a geo bounding box and a cell size into the mosaic's grid (no GPU, no context).
Expected values are worked out by hand: the integer cell numbers are written down, the origin is that number times the cell."""
import math
import pytest

E_ARG = -2


def _grid(bbox, cell):
    from diasss_amd import capi
    p = capi.mosaic_grid(bbox, cell)
    return p.x0, p.y0, p.cell, p.W, p.H, p.use_mask


@pytest.mark.parametrize("bbox,cell,kx,ky,W,H", [
    # xmax = 1.0 lies exactly on the edge between cells 1 and 2: it belongs to cell 2, so three columns; ymax = 2.0 likewise
    ((0.0, 1.0, 0.0, 2.0), 0.5, 0, 0, 3, 5),
    # 0.12 / 0.05 = 2.4 -> cell 2; (0.31 - 0.10) / 0.05 = 4.2 -> 5 columns; -0.26 / 0.05 = -5.2 -> cell -6; (-0.11 + 0.30) / 0.05 = 3.8 -> 4 rows
    ((0.12, 0.31, -0.26, -0.11), 0.05, 2, -6, 5, 4),
    # -0.5 / 0.13 = -3.85 -> cell -4 (origin -0.52); 1.02 / 0.13 = 7.85 -> 8 columns; 1.0 / 0.13 = 7.69 -> cell 7 (0.91); 0.34 / 0.13 = 2.6 -> 3 rows
    ((-0.5, 0.5, 1.0, 1.25), 0.13, -4, 7, 8, 3),
    # negative on both axes: -1.3 / 1.7 = -0.76 -> cell -1; (2.2 + 1.7) / 1.7 = 2.29 -> 3 columns; -0.7 / 1.7 -> cell -1; 2.1 / 1.7 = 1.24 -> 2 rows
    ((-1.3, 2.2, -0.7, 0.4), 1.7, -1, -1, 3, 2),
    # a box wholly below zero: -9.0 / 1.7 = -5.29 -> cell -6 (origin -10.2); (-8.0 + 10.2) / 1.7 = 1.29 -> 2 columns; one point in y
    ((-9.0, -8.0, -3.0, -3.0), 1.7, -6, -2, 2, 1),
])
def test_grid_hand_computed(bbox, cell, kx, ky, W, H):
    x0, y0, c, w, h, use_mask = _grid(bbox, cell)
    assert c == cell and use_mask == 1
    assert x0 == kx * cell and y0 == ky * cell
    assert (w, h) == (W, H)
    # the corners of the box fall into the first and the last cell
    assert math.floor((bbox[0] - x0) / cell) == 0 and math.floor((bbox[1] - x0) / cell) == W - 1
    assert math.floor((bbox[2] - y0) / cell) == 0 and math.floor((bbox[3] - y0) / cell) == H - 1


@pytest.mark.parametrize("cell", [0.0, -0.1, float("nan"), float("inf")])
def test_grid_rejects_bad_cell(cell):
    from diasss_amd import capi
    with pytest.raises(capi.DsssError) as ei:
        capi.mosaic_grid((0.0, 1.0, 0.0, 1.0), cell)
    assert ei.value.code == E_ARG


def test_grid_cell_cap():
    """W H may reach 2^28 and not exceed it"""
    from diasss_amd import capi
    p = capi.mosaic_grid((0.0, 16383.0, 0.0, 16383.0), 1.0)
    assert p.W == 16384 and p.H == 16384
    with pytest.raises(capi.DsssError) as ei:
        capi.mosaic_grid((0.0, 16384.0, 0.0, 16383.0), 1.0)
    assert ei.value.code == E_ARG
    with pytest.raises(capi.DsssError) as ei:
        capi.mosaic_grid((0.0, 1.0e6, 0.0, 1.0e6), 0.05)
    assert ei.value.code == E_ARG


def test_grid_rejects_bad_box():
    from diasss_amd import capi
    for bbox in ((0.0, float("nan"), 0.0, 1.0), (0.0, float("inf"), 0.0, 1.0), (1.0, 0.0, 0.0, 1.0)):
        with pytest.raises(capi.DsssError) as ei:
            capi.mosaic_grid(bbox, 0.5)
        assert ei.value.code == E_ARG
