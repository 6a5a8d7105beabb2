"""NumPy restatement of nerf_occupancy_age (include/nerf_mi355x.h), from the three lines of its
definition.  A helper for the tests, not a test:
    hit(p) = field[p] > level || isnan(field[p])
    age[p] = hit ? 0 : (age[p] == 255 ? 255 : age[p] + 1)
    on[p]  = age[p] < hold ? 1.0f : -1.0f"""
import numpy as np


def new_age(n_points):
    """The state before the first refresh: 255 everywhere."""
    return np.full(n_points, 255, dtype=np.uint8)


def age_step(field, level, hold, age):
    """field: any shape, float32; age: uint8 with field.size entries -> (the new age, on), both flat; `age` is left unchanged."""
    f = np.asarray(field, dtype=np.float32).reshape(-1)
    age = np.asarray(age)
    assert age.dtype == np.uint8 and age.shape == f.shape and 1 <= hold <= 255
    with np.errstate(invalid="ignore"):
        hit = (f > np.float32(level)) | np.isnan(f)
    older = np.where(age == 255, 255, age.astype(np.int32) + 1)
    out = np.where(hit, 0, older).astype(np.uint8)
    on = np.where(out.astype(np.int32) < hold, np.float32(1.0), np.float32(-1.0)).astype(np.float32)
    return out, on
