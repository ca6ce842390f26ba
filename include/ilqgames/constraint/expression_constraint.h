// No counterpart in the reference (a user-defined constraint is a Constraint subclass there): ExpressionConstraint, the
// formula-defined constraint that runs on the device.  The mirrored declarations live in one header.
#include <ilqgames/host/api.hpp>
