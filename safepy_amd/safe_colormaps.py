"""safepy/safe_colormaps.py: the colour helpers of the plot methods.  This module imports matplotlib; `import safepy_amd`
does not import it (the plot methods do, when they run)."""
import matplotlib
import matplotlib.colors as colors
import numpy as np


class MidpointRangeNormalize(colors.Normalize):
    """safe_colormaps.py:8-18: piecewise-linear map of [vmin, midrange[0], midrange[1], midrange[2], vmax] onto
    [0, 0.25, 0.5, 0.75, 1]."""

    def __init__(self, vmin=None, vmax=None, midrange=None, clip=False):
        self.midrange = midrange
        colors.Normalize.__init__(self, vmin, vmax, clip)

    def __call__(self, value, clip=None):
        knots = [self.vmin, *self.midrange[:3], self.vmax]
        return np.ma.masked_array(np.interp(value, knots, [0, 0.25, 0.5, 0.75, 1]))


def get_colors(colormap='hsv', n=10):
    """safe_colormaps.py:21-34: [n, 4] RGBA, black first, then cmap(c / n) for c = 1 .. n-1, those shuffled with NumPy's
    global stream (np.random.shuffle), as the reference does.  The reference's cm.get_cmap(name) is
    matplotlib.colormaps[name] in current matplotlib (cm.get_cmap was removed in 3.9); the colours are the same."""
    cmap = matplotlib.colormaps[colormap]
    rgba = np.asarray([(0, 0, 0, 1)] + [cmap(k / n) for k in range(1, n)])
    np.random.shuffle(rgba[1:])              # the view: the first row stays black
    return rgba
