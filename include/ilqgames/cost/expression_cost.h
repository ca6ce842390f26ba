// No counterpart in the reference (a user-defined cost is a Cost subclass there): host::Expr and ExpressionCost, the
// formula-defined cost that runs on the device.  The mirrored declarations live in one header.
#include <ilqgames/host/api.hpp>
