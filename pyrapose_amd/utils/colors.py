"""Label colours from a generated palette: label -> a hue, at full saturation and value, all in integers.  The reference's
utils/colors.py holds a table of 80 colours; this is not that table, only its interface (label_color(label) -> three values
0..255): consecutive labels step 137 degrees round the colour circle (coprime with 360: the first 360 labels get 360 different
hues, and neighbours in label are far apart in hue)."""

HUE_STEP = 137


def hue_color(h):
    """hue in degrees (any integer) -> (r, g, b) at full saturation and value, integer arithmetic"""
    h = int(h) % 360
    sector, f = divmod(h, 60)
    up = (f * 255 + 30) // 60   # rising edge of the sector
    down = 255 - up
    return ((255, up, 0), (down, 255, 0), (0, 255, up), (0, down, 255), (up, 0, 255), (255, 0, down))[sector]


def label_color(label):
    """the colour of an integer label >= 0 as (r, g, b), each 0..255"""
    label = int(label)
    if label < 0:
        raise ValueError("label_color: label %d is negative" % label)
    return hue_color(label * HUE_STEP)


def id_palette(alpha=255):
    """256 (r, g, b, alpha) rows for an id image: id k >= 1 is label k - 1 (scene_gt_info's instance ids and the mask head's
    arg-max image both keep 0 for the background, which is never drawn)"""
    return [(0, 0, 0, 0)] + [label_color(k - 1) + (int(alpha),) for k in range(1, 256)]
