"""numpy restatement of the reference's flow analysis (velocity_analysis.py), the oracle of the
GPU tests: the reference module itself is not available where those run.

tests/test_flow_oracle.py holds it to fixtures written by the reference (tests/golden/flow_*.npz,
make_flow_golden.py), bit for bit.  The derivatives restate np.gradient with scalar spacings and
edge_order = 1, which is all the reference calls (velocity_analysis.py:34-36, :107-109):

    interior   (f[i+1] - f[i-1]) / (2. * h)
    faces      (f[1] - f[0]) / h,  (f[n-1] - f[n-2]) / h

in the array's dtype (integers as float64), so that a Python-float spacing divides float32 fields in
float32 and a np.float64 spacing divides them in float64, rounded to float32 on assignment.
"""
import numpy as np

TOO_SMALL = ("Shape of array too small to calculate a numerical gradient, at least (edge_order + 1) elements "
             "are required.")
OUTPUTS = ("strain_rate", "dissipation", "vorticity", "flow_type")


def derivative(f, h, axis):
    f = np.asarray(f)
    if f.dtype.kind in "biu":
        f = f.astype(np.float64)
    if f.shape[axis] < 2:
        raise ValueError(TOO_SMALL)

    def at(s):
        return tuple(s if a == axis else slice(None) for a in range(f.ndim))

    out = np.empty_like(f)
    out[at(slice(1, -1))] = (f[at(slice(2, None))] - f[at(slice(None, -2))]) / (2. * h)
    out[at(0)] = (f[at(1)] - f[at(0)]) / h
    out[at(-1)] = (f[at(-1)] - f[at(-2)]) / h
    return out


def gradients(u, v, w, dx, dy, dz):
    """g[field][axis] with axis 0, 1, 2 = x, y, z (array axes 2, 1, 0)."""
    return [[derivative(f, h, ax) for h, ax in ((dx, 2), (dy, 1), (dz, 0))] for f in (u, v, w)]


def strain_rate_of(g):
    (ux, uy, uz), (vx, vy, vz), (wx, wy, wz) = g
    exx, eyy, ezz = 2 * ux, 2 * vy, 2 * wz            # velocity_analysis.py:41-43
    exy, exz, eyz = uy + vx, uz + wx, vz + wy          # :44-46
    return np.sqrt(((0.5 * ((exx * exx + eyy * eyy) + ezz * ezz) + exy * exy) + exz * exz) + eyz * eyz)  # :53-56


def vorticity_of(g):
    (ux, uy, uz), (vx, vy, vz), (wx, wy, wz) = g
    ox, oy, oz = wy - vz, uz - wx, vx - uy             # :111-113
    return np.sqrt((ox * ox + oy * oy) + oz * oz)      # :115


def _masked(a, mask):
    if mask is not None:
        a[~mask] = 0.0
    return a


def compute_strain_rate(u, v, w, dx, dy, dz, mask=None):
    return _masked(strain_rate_of(gradients(u, v, w, dx, dy, dz)), mask)


def compute_vorticity(u, v, w, dx, dy, dz, mask=None):
    return _masked(vorticity_of(gradients(u, v, w, dx, dy, dz)), mask)


def compute_viscous_dissipation(strain_rate, viscosity, dx=1.0, dy=1.0, dz=1.0, mask=None):
    return _masked(viscosity * (strain_rate * strain_rate), mask)  # :85


def compute_astarita_flow_type(strain_rate, vorticity_mag, mask=None):
    num, den = strain_rate - vorticity_mag, strain_rate + vorticity_mag  # :174-175
    out = np.zeros_like(strain_rate)
    safe = den > 1e-15                                                   # :182
    out[safe] = num[safe] / den[safe]
    return _masked(out, mask)


def permeability_from_means(u_mean, v_mean, w_mean, mean_dissipation, viscosity):
    """:138-149 from the four means."""
    darcy = np.sqrt(u_mean**2 + v_mean**2 + w_mean**2)
    if mean_dissipation == 0:
        return 0.0
    return (viscosity * darcy**2) / mean_dissipation


def compute_permeability(u, v, w, dissipation, viscosity, dx, dy, dz, mask=None):
    return permeability_from_means(np.mean(u), np.mean(v), np.mean(w), np.mean(dissipation), viscosity)


def analyze(u, v, w, dx, dy, dz, viscosity, mask=None):
    """The four fields as the reference's functions chained the way analyze_flow.py chains them."""
    s = compute_strain_rate(u, v, w, dx, dy, dz, mask)
    o = compute_vorticity(u, v, w, dx, dy, dz, mask)
    return {"strain_rate": s, "dissipation": compute_viscous_dissipation(s, viscosity, dx, dy, dz, mask),
            "vorticity": o, "flow_type": compute_astarita_flow_type(s, o, mask)}


# ---- fixtures ----
def load_case(path):
    """A fixture as a dict: fields, mask (None when the case has none), spacings of the stored kind
    (Python float or np.float64), the Python-float viscosity and the reference's results."""
    z = np.load(path, allow_pickle=False)
    kind = np.float64 if int(z["strong"]) else float
    case = {k: z[k] for k in ("u", "v", "w") + OUTPUTS}
    case["mask"] = z["mask"] if "mask" in z.files else None
    case["dx"], case["dy"], case["dz"] = (kind(h) for h in z["spacing"])
    case["viscosity"] = float(z["viscosity"])
    case["permeability"] = z["permeability"][()]
    return case


def same(a, b):
    """Equal dtype, shape and values (a NaN equals a NaN)."""
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b, equal_nan=True)
