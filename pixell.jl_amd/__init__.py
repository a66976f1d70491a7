"""pixell.jl_amd -- MI355X-native (gfx950) implementation of the Pixell.jl CAR pixel<->sky hot path.

Host-side mirror of the reference's Enmap/WCS interface (same names, argument meaning and `safe`
behaviour as /root/reference/src/Pixell.jl:35-43 exports for this path) over libpixell_hip.so, a C-ABI
library of hand-written HIP kernels (include/pixell_hip.h).  PyTorch only supplies device memory,
streams and torch.distributed.  The directory name contains a dot, so import it through the
repo-root shim:  `import pixell_jl_amd as pj`.
"""
from . import _lib
from ._lib import PixellHipError, LIB_PATH
from .wcs import (AbstractCARWCS, CarClenshawCurtis, CarFejer1, Gnomonic, SkyBoundingBox, getcdelt, getcrpix,
                  getcrval, getunit, is_periodic, jl_mod, rewind, sliced_wcs)
from .geometry import (JlRange, create_car_wcs, extent_cyl, fullsky_geometry, geometry, laxes_cyl, pad_geometry,
                       skyarea, slice_geometry)
from .enmap import Enmap, NoWCS, getwcs
from .ops import (ApproxSeqSDT, BruteForceSDT, ExactSeqSDT, GenericReprojectPlan, ReprojectPlan, SamplePairs, distance_transform,
                  fill_random_, fill_sphere_points_, pix2sky, pix2sky_, pix2sky_rewind,
                  pixareamap, pixareamap_, posmap, reproject, rewind_, sample, sample_bilinear, sample_pol, scatter, scatter_bilinear, scatter_cubic,
                  scatter_pol, scatter_pol_weights, pol_block_solve, pol_block_apply, normal_pol,
                  sample_nearest, scatter_nearest, sample_pol_nearest, scatter_pol_nearest, scatter_pol_weights_nearest, bin_pol_nearest,
                  baseline_bin_pol_nearest, baseline_project_pol_nearest, polyfilter_tod, modefilter_tod, common_mode_tod,
                  bin_plan, binfilter_tod, scan_bins, toeplitz_tod, noise_kernel_from_psd,
                  autocov_tod, noise_psd_from_autocov, noise_kernel_from_tod,
                  expand_pointing, quat_conj, quat_from_radec, quat_mul,
                  sky2pix, sky2pix_, sky2pix_broadcast, spline_prefilter, spline_prefilter_transpose, unwind_)
from .mapmaker import (binned_map_pol, binned_map_pol_nearest, binned_map_pol_nearest_tod, cg_map_pol, cg_map_pol_tod, destripe_map_pol_nearest_tod,
                       filter_bin_map_pol_nearest_tod, ml_map_pol_nearest_tod, ml_map_pol_nearest_tod_auto, pcg, template_bin_map_pol_nearest_tod)
from .sharding import DecStripLayout, DecStripReprojector, strip_bounds
from .placement import (allocation_policy, empty_map, last_allocation_info, map_classes, place_pair, place_pair_compact, place_pair_native, place_pair_shifted, place_streams,
                        set_allocation_policy)
from .fits_io import read_header, read_map, read_map_rows, wcs_from_header, write_map

# unit shortcuts, Pixell.jl:46-48 (angles are plain radians here)
import math as _math
radian = 1.0
degree = _math.pi / 180
arcminute = _math.pi / 180 / 60


def library_path():
    return LIB_PATH


def load_library():
    """Load libpixell_hip.so now (raises ImportError if it has not been built)."""
    return _lib.load()
