"""What the settings modules share (normal_geo, photometric, multiview, multiview_occlusion, postprocess, reconstruct): the lookup of a configuration block and the
validators of its values.  Each module keeps its Settings, its DEFAULTS and the rules only it has; every refusal is a ValueError
'<block>.<key> must be <what>, got <value>'."""
INF = float('inf')


def is_number(v):
    """A finite int or float; a bool is neither."""
    return not isinstance(v, bool) and isinstance(v, (int, float)) and v == v and v not in (INF, -INF)


class Block(object):
    """The block `name` as the attribute `attr` of `owner` holds it: a dict, an attribute object or None (missing: every key takes its
    default).  Anything else is refused."""

    def __init__(self, owner, attr, name, defaults):
        self.block, self.name, self.defaults = getattr(owner, attr, None), name, defaults
        if self.block is not None and not isinstance(self.block, dict) and not hasattr(self.block, '__dict__'):
            raise ValueError('%s must be a block of keys, got %r' % (name, self.block))

    def get(self, key):
        default = getattr(self.defaults, key)
        if self.block is None:
            return default
        if isinstance(self.block, dict):
            return self.block.get(key, default)
        return getattr(self.block, key, default)

    def refuse(self, key, what, value):
        raise ValueError('%s.%s must be %s, got %r' % (self.name, key, what, value))

    def switch(self, key):
        v = self.get(key)
        if not isinstance(v, bool):
            self.refuse(key, 'true or false', v)
        return v

    def number(self, key, what='a finite number', ok=None):
        """ok: a further condition on the number, which `what` words."""
        v = self.get(key)
        if not is_number(v) or (ok is not None and not ok(v)):
            self.refuse(key, what, v)
        return float(v)

    def positive(self, key, what='a positive finite number'):
        return self.number(key, what, lambda v: v > 0)

    def integer(self, key, allowed, what):
        """allowed: a container of the integers that pass (a tuple, a range)."""
        v = self.get(key)
        if isinstance(v, bool) or not isinstance(v, int) or v not in allowed:
            self.refuse(key, what, v)
        return v
