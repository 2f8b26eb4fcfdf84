"""pyshepseg_amd -- MI355X-native drop-in for the pyshepseg segmentation hot path.

``shepseg``      per-tile Shepherd segmentation (k-means -> clump -> elimination) on HIP
``tiling``       tiled driver + cross-tile stitch
``tilingstats``  per-segment statistics
``utils``        colour tables from per-segment columns, RGBA rendering of the labels
``neighbours``   per-segment neighbour lists and border lengths from the label raster, columns reduced over
                 them, touching segments of one class merged into one
"""
__version__ = '0.1.0'
