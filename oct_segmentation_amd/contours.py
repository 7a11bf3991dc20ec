"""Mask outlines on the GPU: the CRACK CONTOURS of every (slice, channel) plane of a mask stack (``csrc/contours.hip``,
``octseg_stack_contour_counts`` / ``octseg_stack_contours``).

A crack contour is the closed polygon along the pixel SIDES between a set and a clear pixel.  Pixel ``(y, x)`` covers the square
``[x, x + 1] x [y, y + 1]``, vertices are the lattice points ``0 <= x <= W``, ``0 <= y <= H``, the set pixels lie on the right of the direction
of travel (outer contours run clockwise on screen, holes counter-clockwise), diagonal pixels are connected (8-connected foreground, as
``cleanup.label_stack``), and a vertex is listed only where the direction changes.  The polygons are unique, integer, and their even-odd fill at
the pixel centres ``(x + .5, y + .5)`` IS the mask.  This is NOT ``cv2.findContours`` (pixel-centre borders in OpenCV's following order) and not
``skimage.measure.find_contours`` (half-pixel marching squares); ``include/octseg.h`` states the definitions.

    counts = count_stack(stack)                    # int64 CUDA [N, C, 2]: crack edges (= shape.moments_stack's EDGES), contour vertices
    cont = trace_stack(stack)                      # Contours(ncont [N, C], table [K, 10], vertices [V, 2]) on the device
    polys = cont.polygons()                        # host: per slice, per channel, a list of {'label', 'exterior', 'interior', ...}
    shapes = component_shapes(stack)               # per component: area, perimeter, holes, Euler number
    report = contour_report(stack, names, classes) # JSON-ready; svg_frame(polys[i], (w, h), classes) draws one frame

``stack`` is float32 CUDA [N, H, W, channels], any value != 0 set.  Everything is integer; results EQUAL ``tests/contours_ref.py``.
"""
from collections import namedtuple

import numpy as np
import torch

from . import _lib as L
from .cleanup import DEFAULT_SCRATCH, _check

FIELDS = ('plane', 'first_vertex', 'vertices', 'area', 'edges', 'x0', 'y0', 'x1', 'y1', 'label')
NFIELDS = len(FIELDS)
MAX_VERTICES = 1 << 29
CONVENTION = ('crack contours: pixel (y, x) covers [x, x+1] x [y, y+1]; vertices are integer lattice points [x, y] with 0 <= x <= width, '
              '0 <= y <= height; rings are closed implicitly, list corners only, keep the set pixels on the right (exterior clockwise on '
              'screen, interior counter-clockwise); diagonal pixels are connected; the even-odd fill at pixel centres (x + 0.5, y + 0.5) '
              'reproduces the mask; not cv2.findContours and not skimage.measure.find_contours')


def _check_contours(stack):
    stack, n, h, w, sc = _check(stack)
    if (h + 1) * (w + 1) >= MAX_VERTICES:
        raise ValueError(f'frame {h} x {w} has 2^29 vertices or more')
    return stack, n, h, w, sc


def _host(t):
    return t.cpu().numpy() if torch.is_tensor(t) else np.asarray(t)


def count_stack(stack):
    """int64 CUDA [N, channels, 2]: the crack edges of every plane (its perimeter along pixel sides, ``shape.moments_stack``'s ``EDGES``) and
    the number of contour vertices.  One pass over the stack, no scratch, no host synchronisation."""
    stack, n, h, w, sc = _check_contours(stack)
    counts = torch.empty((n, sc, 2), dtype=torch.int64, device=stack.device)
    with torch.cuda.device(stack.device):
        L.check(L.lib().octseg_stack_contour_counts(L.ptr(stack), n, h, w, sc, L.ptr(counts), L.stream_ptr()))
    return counts


def _slices_per_chunk(edges, h, w, sc, scratch_bytes):
    """Slices a call may take under the scratch budget, given the edges of every slice (host list): the largest step whose worst chunk fits;
    1 where not even one slice does (a slice is never split)."""
    n, step = len(edges), len(edges)
    while True:
        worst = max(sum(edges[i:i + step]) for i in range(0, n, step))
        need = int(L.lib().octseg_contours_scratch_bytes(step * sc, h, w, max(worst, 1)))
        if step == 1 or 0 < need <= scratch_bytes:
            return step
        step = max(1, min(step - 1, step * int(scratch_bytes) // max(need, 1)))


class Contours(namedtuple('Contours', ('ncont', 'table', 'vertices', 'size'), defaults=(None,))):
    """``ncont`` int32 [N, channels], ``table`` int32 [K, 10] (columns ``FIELDS``; K = ncont.sum(), ordered by plane then leader), ``vertices``
    int32 [V, 2] = x, y, ``size`` = (W, H) or None where the frame size is not known.  Device tensors from ``trace_stack``; numpy arrays work as well (the host methods take either)."""
    __slots__ = ()

    def polygons(self):
        """Host: ``[slice][channel]`` -> list of ``{'label', 'exterior': [[x, y], ...], 'interior': [[[x, y], ...], ...], 'area', 'perimeter',
        'holes', 'bbox'}``, one per component in label order (= first pixel in raster order).  Holes hang on the exterior with their label;
        ``area`` = exterior minus holes = the component's pixel count, ``perimeter`` = the crack edges of exterior and holes, ``bbox`` =
        ``[x0, y0, x1, y1]`` of the exterior on the vertex lattice."""
        ncont, table, verts = _host(self.ncont), _host(self.table), _host(self.vertices)
        n, sc = ncont.shape
        out = [[[] for _ in range(sc)] for _ in range(n)]
        by_label = {}
        vl = verts.tolist()
        for row in table.tolist():
            plane, first, nv, area, edges, x0, y0, x1, y1, label = row
            ring = vl[first:first + nv]
            if area > 0:
                poly = {'label': label, 'exterior': ring, 'interior': [], 'area': area, 'perimeter': edges, 'holes': 0, 'bbox': [x0, y0, x1, y1]}
                out[plane // sc][plane % sc].append(poly)
                by_label[(plane, label)] = poly
        for row in table.tolist():
            plane, first, nv, area, edges, label = row[0], row[1], row[2], row[3], row[4], row[9]
            if area < 0:
                poly = by_label[(plane, label)]
                poly['interior'].append(vl[first:first + nv])
                poly['area'] += area
                poly['perimeter'] += edges
                poly['holes'] += 1
        return out

    def shapes(self):
        """Host: ``[slice][channel]`` -> list of ``{'label', 'area', 'perimeter', 'holes', 'euler', 'bbox'}`` per component, ordered as
        ``cleanup.component_table`` ranks them (area descending, first pixel ascending).  ``euler`` = 1 - holes."""
        out = []
        for frame in self.polygons():
            out.append([sorted(({'label': p['label'], 'area': p['area'], 'perimeter': p['perimeter'], 'holes': p['holes'],
                                 'euler': 1 - p['holes'], 'bbox': p['bbox']} for p in polys), key=lambda s: (-s['area'], s['label']))
                        for polys in frame])
        return out


def trace_stack(stack, scratch_bytes=DEFAULT_SCRATCH):
    """Trace every plane: ``Contours`` on the device.  One ``count_stack`` call and one host read of its per-slice sums size the buffers
    exactly (edges, vertices; contours at most edges // 4); the slices are traced in chunks whose scratch stays under ``scratch_bytes`` (one
    chunk when it fits; slice by slice when not even one fits) and the result does not depend on the chunking.  One more host read at the end
    fetches the overflow flag and the contour totals; an overflow raises."""
    stack, n, h, w, sc = _check_contours(stack)
    dev = stack.device
    sums = count_stack(stack).sum(dim=1).cpu().tolist()                     # [N][2]
    edges, nverts = [int(s[0]) for s in sums], [int(s[1]) for s in sums]
    step = _slices_per_chunk(edges, h, w, sc, scratch_bytes)
    starts = list(range(0, n, step))
    ecap = [max(sum(edges[i:i + step]), 1) for i in starts]
    ccap = [max(e // 4, 1) for e in ecap]
    vcap = [max(sum(nverts[i:i + step]), 1) for i in starts]
    if max(ecap) >= 2 ** 31:
        raise ValueError('a slice has 2^31 crack edges or more')
    ncont = torch.empty((n, sc), dtype=torch.int32, device=dev)
    table = torch.empty((sum(ccap), NFIELDS), dtype=torch.int32, device=dev)
    verts = torch.empty((sum(vcap), 2), dtype=torch.int32, device=dev)
    overflow = torch.zeros((1,), dtype=torch.int32, device=dev)
    lib = L.lib()
    with torch.cuda.device(dev):
        need = max(int(lib.octseg_contours_scratch_bytes(min(step, n - i) * sc, h, w, e)) for i, e in zip(starts, ecap))
        scratch = torch.empty((need,), dtype=torch.uint8, device=dev)
        c0 = v0 = 0
        for i, e, c, v in zip(starts, ecap, ccap, vcap):
            m = min(step, n - i)
            L.check(lib.octseg_stack_contours(L.ptr(stack[i:i + m]), m, h, w, sc, L.ptr(scratch), need, e, c, v, L.ptr(ncont[i:i + m]),
                                              L.ptr(table[c0:c0 + c]), L.ptr(verts[v0:v0 + v]), L.ptr(overflow), L.stream_ptr()))
            c0, v0 = c0 + c, v0 + v
    per_chunk = torch.stack([ncont[i:i + step].sum() for i in starts])
    host = torch.cat([overflow.to(torch.int64), per_chunk]).cpu().tolist()
    if host[0]:
        raise RuntimeError('octseg_stack_contours reported an overflow of capacities sized by octseg_stack_contour_counts')
    if len(starts) == 1:
        return Contours(ncont, table[:host[1]], verts[:sum(nverts)], (w, h))
    rows, lists, c0, v0, vrun = [], [], 0, 0, 0
    for i, c, v, k in zip(starts, ccap, vcap, host[1:]):                      # a chunk's planes and vertices start at 0: move them into place
        tv = sum(nverts[i:i + step])                                          # (v is tv, or a one-row placeholder where tv is 0)
        part = table[c0:c0 + k].clone()
        part[:, 0] += i * sc
        part[:, 1] += vrun
        rows.append(part)
        lists.append(verts[v0:v0 + tv])
        c0, v0, vrun = c0 + c, v0 + v, vrun + tv
    return Contours(ncont, torch.cat(rows), torch.cat(lists), (w, h))


def _as_contours(stack_or_contours, scratch_bytes=DEFAULT_SCRATCH):
    return stack_or_contours if isinstance(stack_or_contours, Contours) else trace_stack(stack_or_contours, scratch_bytes)


def component_shapes(stack):
    """Per component of every plane its pixel area, perimeter (crack edges of its exterior and its holes), hole count and Euler number
    1 - holes, with the exterior's vertex-lattice box: ``Contours.shapes()`` of the traced stack (a ``Contours`` is taken as it is).  The areas
    and the order are those of ``cleanup.component_table``, which lists the first 8."""
    return _as_contours(stack).shapes()


def default_classes(channels):
    from .lesions import default_classes as dc
    return dc(channels)


def contour_report(stack, names=None, classes=None):
    """JSON-ready: ``{'convention', 'width', 'height', 'classes', 'slices': [{'name', 'objects': {class: [polygon, ...]}}]}`` with the
    polygons of ``Contours.polygons()``; ``stack`` may be a ``Contours``.  ``names`` default to ``'0', '1', ...``; ``classes`` to the project's
    class order."""
    cont = _as_contours(stack)
    polys = cont.polygons()
    n = len(polys)
    sc = len(polys[0]) if n else 0
    names = [str(i) for i in range(n)] if names is None else [str(s) for s in names]
    if len(names) != n:
        raise ValueError(f'{len(names)} names for {n} slices')
    classes = default_classes(sc) if classes is None else [str(c) for c in classes]
    if len(classes) != sc:
        raise ValueError(f'{len(classes)} class names for {sc} channels')
    w, h = (int(v) for v in cont.size) if cont.size is not None else (None, None)
    return {'convention': CONVENTION, 'width': w, 'height': h, 'classes': list(classes),
            'slices': [{'name': name, 'objects': {cls: polys[i][c] for c, cls in enumerate(classes)}} for i, name in enumerate(names)]}


def _class_colours(classes):
    from .postprocess import CLASS_COLORS_RGB
    return ['#%02x%02x%02x' % tuple(CLASS_COLORS_RGB.get(str(cls), (128, 128, 128))) for cls in classes]      # (grey: a channel without a class)


def svg_frame(polygons, size, classes):
    """One frame as SVG text: ``polygons`` is ``Contours.polygons()[i]`` (a list per channel), ``size`` = (width, height), ``classes`` the
    channel names.  One ``<path fill-rule="evenodd">`` per class in the class colour, every ring an ``M x y L ... Z`` subpath: the even-odd
    rule cuts the holes, and integer coordinates on the pixel lattice make the drawing the mask itself."""
    w, h = (int(v) for v in size)
    if len(polygons) != len(classes):
        raise ValueError(f'{len(polygons)} channels for {len(classes)} class names')
    lines = [f'<svg xmlns="http://www.w3.org/2000/svg" width="{w}" height="{h}" viewBox="0 0 {w} {h}" shape-rendering="crispEdges">']
    for polys, cls, colour in zip(polygons, classes, _class_colours(classes)):
        rings = [r for p in polys for r in [p['exterior']] + p['interior']]
        d = ' '.join('M ' + ' L '.join(f'{x} {y}' for x, y in ring) + ' Z' for ring in rings)
        lines.append(f'<path id="{cls}" fill="{colour}" fill-opacity="0.5" stroke="{colour}" stroke-width="0.5" fill-rule="evenodd" d="{d}"/>')
    lines.append('</svg>')
    return '\n'.join(lines)
