"""NumPy restatement of the mesh clean-up definitions of DESIGN.md section 2.11 (include/nerf_mi355x.h, nerf_mesh_components and
nerf_mesh_filter_*) for the tests to compare with exactly.  A helper, not a test.  No concurrent union-find here: whole-array rounds
that propagate the minimum label over the faces until no face has corners with different labels."""
import numpy as np


def components_reference(faces, n_vertices):
    """-> vertex_label [V] int32, face_label [T] int32, (comp_label, comp_faces, comp_vertices) [C] int32, ascending label."""
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    V = int(n_vertices)
    ok = ((f >= 0) & (f < V)).all(axis=1)                       # a face with an index out of range joins nothing
    g = f[ok]
    label = np.arange(V, dtype=np.int64)                       # label[v] <= v, a vertex id of v's component
    todo = g
    while len(todo):
        lab = label[todo]
        low = lab.min(axis=1)
        open_ = lab.max(axis=1) != low                          # faces whose corners all share a label are done for good (see below)
        todo, lab, low = todo[open_], lab[open_], low[open_]
        for c in range(3):
            np.minimum.at(label, lab[:, c], low)                 # labels are vertex ids: the higher label goes under the lowest
        while True:                                              # ... and every vertex follows its label down to where label[l] == l,
            nxt = label[label]                                   # so two vertices that once shared a label share one ever after
            if np.array_equal(nxt, label):
                break
            label = nxt
    face_label = np.full(len(f), -1, dtype=np.int64)
    face_label[ok] = label[g[:, 0]]
    comp_label = np.flatnonzero(label == np.arange(V))
    comp_faces = np.bincount(face_label[ok], minlength=V)[comp_label] if V else np.zeros(0, np.int64)
    comp_vertices = np.bincount(label, minlength=V)[comp_label] if V else np.zeros(0, np.int64)
    return label.astype(np.int32), face_label.astype(np.int32), tuple(a.astype(np.int32) for a in (comp_label, comp_faces, comp_vertices))


def select_reference(table, min_triangles=None, keep_largest=None):
    """The labels of the kept components: at least min_triangles faces, and among the keep_largest with the most faces (ties: the
    smaller label first)."""
    label, n_faces, _ = table
    kept = set(label.tolist())
    if min_triangles is not None:
        kept &= {int(l) for l, n in zip(label, n_faces) if n >= min_triangles}
    if keep_largest is not None:
        ranked = sorted(zip(label.tolist(), n_faces.tolist()), key=lambda r: (-r[1], r[0]))
        kept &= {l for l, _ in ranked[:keep_largest]}
    return kept


def filter_reference(vertices, faces, min_triangles=None, keep_largest=None, components=None):
    """-> vertices' [V',3], faces' [T',3] int32, vertex_index [V'] int32: the kept components in their original order.
    components: what components_reference gave for this mesh, to spare the recomputation."""
    v = np.asarray(vertices)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    vl, fl, table = components_reference(f, len(v)) if components is None else components
    kept = np.array(sorted(select_reference(table, min_triangles, keep_largest)), dtype=np.int64)
    keep_v, keep_f = np.isin(vl, kept), np.isin(fl, kept)
    index = np.flatnonzero(keep_v)
    new_id = np.full(len(v), -1, dtype=np.int64)
    new_id[index] = np.arange(len(index))
    return v[index], new_id[f[keep_f]].astype(np.int32).reshape(-1, 3), index.astype(np.int32)
