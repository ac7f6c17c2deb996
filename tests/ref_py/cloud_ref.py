"""GridMapRosConverter::toPointCloud restated in numpy (include/travgpu.h has the contract): which cells are emitted, in which
order, and the floats of their records."""
import numpy as np


def cell_positions(rows, cols, resolution, position):
    """float32 x[rows], y[cols] of the cell centres, from grid_map's double arithmetic (te_geom.h: ax + res * (-i))."""
    res = float(resolution)
    ax = float(position[0]) + (0.5 * (rows * res) - 0.5 * res)
    ay = float(position[1]) + (0.5 * (cols * res) - 0.5 * res)
    x = (ax + res * (-np.arange(rows, dtype=np.float64))).astype(np.float32)
    y = (ay + res * (-np.arange(cols, dtype=np.float64))).astype(np.float32)
    return x, y


def to_point_cloud(layers, names, point_layer, rows, cols, resolution, position, basic_layers=()):
    """layers: {name: rows * cols float32 in storage order (element (i, j) at j * rows + i)}; names: the record's layers in
    order.  Returns (field names, float32 [n_points, len(names) + 2])."""
    assert list(names).count(point_layer) == 1
    data = {k: np.asarray(v, dtype=np.float32).reshape(-1) for k, v in layers.items()}
    n = rows * cols
    valid = np.isfinite(data[point_layer])
    for b in basic_layers:
        valid &= np.isfinite(data[b])
    cells = np.nonzero(valid)[0]  # (storage order = GridMapIterator order at start index (0, 0))
    x, y = cell_positions(rows, cols, resolution, position)
    fields, cols_out = [], []
    for name in names:
        if name == point_layer:
            fields += ["x", "y", "z"]
            cols_out += [x[cells % rows], y[cells // rows], data[name][cells]]
        else:
            fields.append(name)
            cols_out.append(data[name][cells])
    assert all(c.dtype == np.float32 for c in cols_out) and n == data[point_layer].size
    return fields, np.stack(cols_out, axis=1) if len(cells) else np.zeros((0, len(fields)), np.float32)
