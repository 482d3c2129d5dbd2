"""Overlay of the reference's `render` package.

The reference's notebooks import its Blender wrapper as `from render.render_point_cloud import render_point_cloud`, with the
reference's `dpc/` directory -- which holds its own regular package `render` (render_point_cloud, the Blender script, the
runner) -- on sys.path.  Put THIS package's parent directory on sys.path BEFORE that one, as for `util` (util/__init__.py),
and `render.render_point_cloud` resolves here (the GPU renderer of dpc.render.visualise), while every other module of the
reference's `render` package keeps resolving to the reference: the package's search path is extended with every other
`render` directory found on sys.path (pkgutil.extend_path), this directory first.  Names the replaced module does not
define fall through to the reference's module of the same name (util/_overlay.py).
"""
from pkgutil import extend_path

__path__ = extend_path(__path__, __name__)
