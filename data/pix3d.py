from shapeclipper_amd.data.pix3d import *  # noqa: F401,F403
from shapeclipper_amd.data.pix3d import Dataset, sample_rays_device  # noqa: F401
