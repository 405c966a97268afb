"""Scene texts and meshes generated at test time, shared by the GPU walk tests (test_gpu_bvh_walks.py) and the CPU
scene-image tests (test_scene_image.py): string edits of the stock scenes and OBJ files (a sine heightfield, single
triangles) that put a BVH on a chosen side of each tier's threshold."""
import os
import re

import numpy as np

from conftest import SCENES


def _xml(name):
    """A stock scene's text with its mesh paths made absolute (load_string has no base directory)."""
    xml = open(os.path.join(SCENES, name)).read()
    return xml.replace('value="meshes/', 'value="%s/meshes/' % SCENES)


def _add(xml, shapes):
    assert "</scene>" in xml
    return xml.replace("</scene>", shapes + "\n</scene>")


def _heightfield_obj(path, n):
    """n x n cells on [-0.5, 0.5]^2, z = 0.05 sin(7 i / n) cos(5 j / n), two triangles per cell."""
    i, j = np.meshgrid(np.arange(n + 1), np.arange(n + 1), indexing="ij")
    x, y = i / n - 0.5, j / n - 0.5
    z = 0.05 * np.sin(7.0 * i / n) * np.cos(5.0 * j / n)
    v = np.stack([x, y, z], axis=-1).reshape(-1, 3)
    ci, cj = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    a = (ci * (n + 1) + cj + 1).ravel()          # 1-based index of vertex (i, j)
    b, c, d = a + (n + 1), a + (n + 2), a + 1    # (i+1, j), (i+1, j+1), (i, j+1)
    f = np.concatenate([np.stack([a, b, c], axis=1), np.stack([a, c, d], axis=1)], axis=1).reshape(-1, 3)
    with open(path, "w") as out:
        out.write("".join("v %.9g %.9g %.9g\n" % tuple(r) for r in v))
        out.write("".join("f %d %d %d\n" % tuple(r) for r in f))
    return len(f)


def _triangle_obj(path):
    with open(path, "w") as out:
        out.write("v 0 0 0\nv 0.2 0 0\nv 0 0.2 0\nf 1 2 3\n")


def _obj_shape(path, transform, bsdf="white"):
    return ('<shape type="obj"><string name="filename" value="%s"/><transform name="to_world">%s</transform>'
            '<ref id="%s"/></shape>' % (path, transform, bsdf))


# three small off-axis rectangles in free space; the second is an area light facing down and into the room
def _extra_rects(n):
    rects = [
        '<shape type="rectangle"><transform name="to_world"><scale value="0.25"/><rotate y="1" angle="35"/>'
        '<rotate x="1" angle="-20"/><translate x="-0.5" y="0.3" z="0.4"/></transform><ref id="white"/></shape>',
        '<shape type="rectangle"><transform name="to_world"><scale value="0.15"/><rotate y="1" angle="-25"/>'
        '<rotate x="1" angle="100"/><translate x="0.5" y="0.6" z="0.0"/></transform><ref id="white"/>'
        '<emitter type="area"><rgb name="radiance" value="12, 12, 12"/></emitter></shape>',
        '<shape type="rectangle"><transform name="to_world"><scale value="0.3"/><rotate y="1" angle="-50"/>'
        '<rotate x="1" angle="15"/><translate x="0.1" y="0.1" z="0.55"/></transform><ref id="green"/></shape>']
    return "\n".join(rects[:n])


def _heightfield_room_xml(tmp_path, n):
    """cbox_mesh.xml with the ball and the ring replaced by one heightfield 1.6 wide above the floor; the six
    walls stay outside the BVH, so the tree is the heightfield's.  Returns (xml, triangles)."""
    obj = str(tmp_path / ("heightfield_%d.obj" % n))
    n_tri = _heightfield_obj(obj, n)
    xml, k = re.subn(r'<shape type="obj" id="ball">.*?</shape>\s*<shape type="ply" id="ring">.*?</shape>',
                     _obj_shape(obj, '<scale value="1.6"/><rotate x="1" angle="-90"/><translate y="-0.8"/>'),
                     _xml("cbox_mesh.xml"), flags=re.S)
    assert k == 1
    return xml, n_tri


def _grid_with_heightfield_xml(tmp_path, n, loose=0):
    """The Cornell box plus an n x n heightfield above the cubes and `loose` single triangles under the ceiling.
    Returns (xml, triangles added)."""
    obj = str(tmp_path / ("heightfield_%d.obj" % n))
    n_tri = _heightfield_obj(obj, n)
    shape = _obj_shape(obj, '<scale value="0.7"/><rotate x="1" angle="-90"/><translate x="0.1" y="0.4" z="0.1"/>')
    if loose:
        tri = str(tmp_path / "triangle.obj")
        _triangle_obj(tri)
        shape += "".join(_obj_shape(tri, '<rotate y="1" angle="%d"/><translate x="%.3f" y="%.3f" z="%.3f"/>' % (
            37 * i, -0.8 + 0.2 * (i % 9), 0.6 + 0.08 * (i // 9), -0.7 + 0.15 * (i % 7))) for i in range(loose))
    return _add(_xml("cbox_grid.xml"), shape), n_tri + loose
